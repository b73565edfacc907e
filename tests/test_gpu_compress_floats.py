"""GPU tests (-m gpu) of compress floats (sprintz_mi355x_compress_batch_float / _float_dense, ChunkedCodec.compress_floats): a float32 /
float16 / bfloat16 source quantised inside the encoders.

The expected value is always the numpy model's q (tests/quant_model.py) of the source on the host: decompress(batch) must be q, and the
container, the offsets, the sizes and the return values must be those of cd.compress(q) -- byte for byte, no tolerance anywhere.  Column d
takes parameter pair d % 8 of the model's list, so a value quantised with another column's parameters shows.  Every launch asserts its
kernel family (tests/dispatch.py) against the planner probe's answer for the shape (tests/plan_probe.cpp), under SPRINTZ_OPT_NO_FAST 0 and 1."""
import ctypes as C
import zlib

import numpy as np
import pytest

import planner
import quant_model as qm
import rle_drive as rd
from dispatch import ran
from drive_tables import NB, NCHUNKS, batch_of as rle_batch_of
from fixtures import no_fast, sz  # noqa: F401  (fixtures)
from harness import DTYPES
from rowdata import GENERIC_SHAPES, gen_data
from streams import check_streams, fire_batch_of

pytestmark = pytest.mark.gpu

FLOAT = planner.QUERY["float"]
CODEC_ID = {"delta": 0, "xff": 1}
PAIR_SHAPES = [(2, 8), (2, 5), (2, 16), (2, 64), (1, 16), (1, 64)]
WIDE_SHAPES = [(2, 80), (2, 128), (1, 128)]
SPLIT_SHAPES = [(1, 80)]
GENERIC = [s for s in GENERIC_SHAPES if s not in PAIR_SHAPES]        # (uint16 x 5 decodes on the generic kernel and encodes on encode_wide.h)
FAMILY = dict([(s, "enc_pair") for s in PAIR_SHAPES] + [(s, "enc_wide") for s in WIDE_SHAPES] + [(s, "enc_split") for s in SPLIT_SHAPES] +
              [(s, "enc_generic") for s in GENERIC])


def rotate(key, k):
    return zlib.crc32(key.encode()) % k


def ask(cd, nchunks, total_len, fmt, fam=0, src_lo=0):
    """the planner's answer for the dense call of this shape -> (encoder family, container family)"""
    planner.available(required=True)
    got = planner.ask("dense", q=FLOAT, out_esz=qm.SRC_BYTES[fmt], codec=CODEC_ID[cd.codec], esz=cd.esz, D=cd.ndims, chunk_len=cd.chunk_len, nchunks=nchunks,
                      total_len=total_len, slot_stride=cd.slot_stride, no_fast=fam, src_lo=src_lo)
    assert "error" not in got and got["family"] in ("dense_fused", "dense_compact"), got
    return got["enc"], got["family"]


def to_tensor(bits, fmt, shift=0):
    """the source on the device (qm.source_bits' array), `shift` elements into a buffer of its own: -> (tensor of the source, its owner)"""
    import torch
    if fmt == qm.F32:
        host = torch.from_numpy(np.ascontiguousarray(bits, np.float32))
    else:
        host = torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16).copy()).view(torch.float16 if fmt == qm.F16 else torch.bfloat16)
    buf = torch.empty(shift + host.numel(), dtype=host.dtype, device="cuda")      # exactly as long as the source: nothing behind it belongs to the call
    buf[shift:] = host.cuda()
    return buf[shift:], buf


def float_dense(cd, src, fmt, inv, off, signed, floor):
    """sprintz_mi355x_compress_batch_float_dense on fresh buffers -> dict(data, offsets, sizes, rets) on the host, data cut at the container's end"""
    import torch
    from sprintz_amd import _lib
    total_len = src.numel()
    n = int(_lib.num_chunks(total_len, cd.chunk_len))
    dev = src.device
    slots = torch.empty(n * cd.slot_stride, dtype=torch.uint8, device=dev)
    sizes = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    rets = torch.full((n + 1,), -77, dtype=torch.int64, device=dev)
    tmp = torch.empty(int(_lib.compress_dense_tmp_bytes(n)), dtype=torch.uint8, device=dev)
    dense = torch.full((n * cd.slot_stride + _lib.READ_SLACK,), 0xEE, dtype=torch.uint8, device=dev)
    offsets = torch.full((n + 2,), -5, dtype=torch.int64, device=dev)
    i = None if inv is None else torch.from_numpy(np.ascontiguousarray(inv, np.float32)).to(dev)
    o = None if off is None else torch.from_numpy(np.ascontiguousarray(off, np.float32)).to(dev)
    flags = (_lib.FLOAT_SIGNED if signed else 0) | (_lib.QUANT_FLOOR if floor else 0)
    _lib.check(_lib.compress_batch_float_dense(CODEC_ID[cd.codec], cd.esz, src.data_ptr(), fmt, None if i is None else i.data_ptr(), None if o is None else o.data_ptr(),
                                               flags, total_len, cd.chunk_len, cd.ndims, slots.data_ptr(), cd.slot_stride, sizes.data_ptr(), rets.data_ptr(),
                                               dense.data_ptr(), offsets.data_ptr(), tmp.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    offs = offsets.cpu().numpy()
    assert offs[n + 1] == -5 and sizes[n].item() == -7 and rets[n].item() == -77, "written behind offsets / sizes / rets"
    total = int(offs[n])
    return dict(data=dense[:total].cpu().numpy(), offsets=offs[:n + 1], sizes=sizes[:n].cpu().numpy(), rets=rets[:n].cpu().numpy(), dense=dense, offs_t=offsets[:n + 1], n=n)


def int_dense(cd, q):
    """cd.compress of the integer tensor q -> the same dict"""
    import torch
    t = torch.from_numpy(q.view(np.int8 if q.dtype.itemsize == 1 else np.int16).copy()).cuda().view(cd.dtype)
    batch = cd.compress(t)
    rets = cd.workspace(batch.nchunks)["rets"].cpu().numpy().copy()
    total = int(batch.offsets[-1].item())
    return dict(data=batch.data[:total].cpu().numpy(), offsets=batch.offsets.cpu().numpy(), sizes=batch.sizes.cpu().numpy(), rets=rets)


def assert_same(sz, cd, got, want, q, tag):
    """the float call's container against cd.compress(q)'s, and its decode against q"""
    import torch
    assert np.array_equal(got["sizes"], want["sizes"]), (tag, "sizes", got["sizes"].tolist()[:8], want["sizes"].tolist()[:8])
    assert np.array_equal(got["rets"], want["rets"]), (tag, "rets", got["rets"].tolist()[:8], want["rets"].tolist()[:8])
    assert np.array_equal(got["offsets"], want["offsets"]), (tag, "offsets")
    ne = np.flatnonzero(got["data"] != want["data"]) if got["data"].size == want["data"].size else None
    assert ne is not None and ne.size == 0, (tag, "container bytes differ; first at", None if ne is None else int(ne[0]))
    n = got["n"]
    batch = sz.CompressedBatch(got["dense"], got["offs_t"], torch.from_numpy(got["sizes"]).cuda(), n, q.size, cd.chunk_len, cd.ndims)
    out = cd.decompress(batch).cpu().numpy().view(DTYPES[cd.esz])[:q.size]
    bad = np.flatnonzero(out != q)
    assert bad.size == 0, (tag, "decode differs from the model; first at element", int(bad[0]), "chunk", int(bad[0]) // cd.chunk_len, int(out[bad[0]]), int(q[bad[0]]))


def same_batch(a, b):
    """two CompressedBatch hold the same container (the bytes behind its end are nobody's)"""
    import torch
    total = int(a.offsets[-1].item())
    return torch.equal(a.offsets, b.offsets) and torch.equal(a.sizes, b.sizes) and torch.equal(a.data[:total], b.data[:total])


def make_values(rng, kind, n, esz, D, chunk_len, inv, off):
    """float64 values whose quantised form is interesting to the encoder: integer data of `kind` (tests/rowdata.py), a fraction added -- ties
    among them --, a few values past both ends of the range, mapped back through column d's parameters"""
    W = 8 * esz
    w = gen_data(kind, rng, n, esz, D).astype(np.float64)
    w = w + rng.choice([0.0, 0.0, 0.25, 0.5, -0.5, 0.49, -0.3], n)
    over = rng.random(n) < 0.01
    w[over] += rng.choice([-(1 << W), 1 << W], int(over.sum()))
    d = (np.arange(n) % chunk_len) % D
    with np.errstate(all="ignore"):
        return w / inv[d].astype(np.float64) + off[d].astype(np.float64)


def run_case(sz, no_fast, codec, esz, D, chunk_len, n, key, want_family=None, values=None):
    """one case: the three formats, signed / unsigned and the rounding by the key, both NO_FAST legs"""
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    W = 8 * esz
    inv, off = qm.column_params(D)
    kind = ("walk", "uniform", "sparse", "constant")[rotate("k" + key, 4)]
    x = make_values(rng, kind, n, esz, D, chunk_len, inv, off) if values is None else values
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device="cuda:0")
    nchunks = -(-n // chunk_len)
    seen = set()
    for j, fmt in enumerate(qm.FORMATS):
        signed, floor = bool((rotate("s" + key, 2) + j) % 2), bool((rotate("f" + key, 4) + j) % 3 == 0)
        bits = qm.source_bits(x, fmt)
        q = qm.compress_floats(qm.source_values(bits, fmt), chunk_len, D, W, inv, off, signed, floor)
        want = int_dense(cd, q)
        src, _owner = to_tensor(bits, fmt)
        for fam in (0, 1):
            no_fast(fam)
            enc, dense = ask(cd, nchunks, n, fmt, fam)
            if want_family is not None:
                assert enc == (want_family if not fam else "enc_generic"), (key, fam, enc)
            seen.add(enc)
            with ran(only=[enc, dense], **{enc: 1, dense: 1}):
                got = float_dense(cd, src, fmt, inv, off, signed, floor)
            assert_same(sz, cd, got, want, q, (key, qm.NAMES[fmt], signed, floor, enc, dense))
        no_fast(0)
    return seen


# ------------------------------------------------------------------ the named shapes

def named_chunk_len(esz, D):
    """about 4 KB of whole groups of 16 rows -- at least two -- and a verbatim tail of 3 rows; where 3 rows are no whole 16-byte pieces
    (uint16 x 5: blocks and chunks of whole pieces are what encode_wide.h takes) a tail of 8 rows, which is verbatim too"""
    tail = 3 if (3 * D * esz) % 16 == 0 or FAMILY[(esz, D)] == "enc_generic" else 8
    return D * (16 * max(2, 4096 // (16 * D * esz)) + tail)


def named_cases():
    return [(codec, esz, D) for codec in ("delta", "xff") for esz, D in PAIR_SHAPES + WIDE_SHAPES + SPLIT_SHAPES + GENERIC]


@pytest.mark.parametrize("codec,esz,D", named_cases())
def test_named_shapes(sz, no_fast, codec, esz, D):
    """5 to 8 chunks of whole groups and a verbatim tail, a short last chunk that ends mid-row: every family a float source has"""
    chunk_len = named_chunk_len(esz, D)
    nchunks = 5 + D % 4
    n = nchunks * chunk_len - (chunk_len // (3 * D)) * D - D // 2
    run_case(sz, no_fast, codec, esz, D, chunk_len, n, f"named{codec}{esz}{D}", FAMILY[(esz, D)])


@pytest.mark.parametrize("codec,esz,D", named_cases())
def test_short_chunks(sz, no_fast, codec, esz, D):
    """13-row chunks -- no group at all: the whole chunk through the encoder's tail, never the verbatim kernel, which copies raw bytes --
    and a batch whose chunks hold fewer than 128 elements"""
    seen = run_case(sz, no_fast, codec, esz, D, 13 * D, 6 * 13 * D - D // 2 - D, f"short{codec}{esz}{D}")
    assert seen == {"enc_generic"}                                                # (encode_wide.h takes chunks of two blocks and more)
    rows = max(1, min(13, 127 // D))
    if rows * D < 128 and rows != 13:
        run_case(sz, no_fast, codec, esz, D, rows * D, 5 * rows * D - max(1, D // 2), f"tiny{codec}{esz}{D}")


@pytest.mark.parametrize("esz,D", [(2, 8), (1, 16), (2, 80), (1, 80)])
def test_short_last_chunk_on_the_wide_kernels(sz, no_fast, esz, D):
    """encode_wide.h's own short paths: a last chunk of fewer than 128 elements (n < 128: the window copy) behind chunks of whole groups,
    and one too short for a group"""
    chunk_len = named_chunk_len(esz, D)
    for last in (max(D, 120 // D * D) - D // 2, 11 * D):
        run_case(sz, no_fast, "xff", esz, D, chunk_len, 4 * chunk_len + last, f"last{esz}{D}{last}", FAMILY[(esz, D)])


# ------------------------------------------------------------------ special values

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 16), ("xff", 1, 80), ("delta", 2, 128), ("xff", 2, 3), ("delta", 1, 7)])
def test_special_values(sz, no_fast, codec, esz, D):
    """NaN, +-inf, -0.0, ties and values out of range in a block's body, in the verbatim tail and in the short last chunk"""
    key = f"special{codec}{esz}{D}"
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    chunk_len = named_chunk_len(esz, D)
    n = 5 * chunk_len + 9 * D + D // 2
    inv, off = qm.column_params(D)
    x = make_values(rng, "walk", n, esz, D, chunk_len, inv, off)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.5, 1.5, 2.5, -0.5, 1e30, -1e30, 3e38, 254.5, 255.5, 65534.5, 65535.5, 127.5, -128.5, 1e-45, -1e-40])
    body = chunk_len - (chunk_len % (16 * D))                                     # where the verbatim tail starts
    for start in (3 * D + 1, 2 * chunk_len + 16 * D + 5, chunk_len + body + 2, 3 * chunk_len + body + D, 5 * chunk_len + 1, n - special.size - 1):
        x[start:start + special.size] = special
    x[2 * chunk_len + 7::97] = np.nan
    run_case(sz, no_fast, codec, esz, D, chunk_len, n, key, FAMILY[(esz, D)], values=x)


# ------------------------------------------------------------------ the drives

# w, D, blocks a chunk, elements behind the last whole block (whole rows): encode_wide.h's mappings and the generic kernel's
RLE_SHAPES = [(16, 8, NB, 0), (8, 6, NB, 0), (8, 32, NB, 0), (8, 80, 51, 0), (8, 96, 48, 0), (16, 80, 48, 0), (8, 5, NB, 35), (8, 1, NB, 7), (16, 2, NB, 14)]
RLE_FAMILY = {(16, 8): "enc_pair", (8, 6): "enc_pair", (8, 32): "enc_pair", (8, 80): "enc_split", (8, 96): "enc_wide", (16, 80): "enc_wide", (8, 5): "enc_generic",
              (8, 1): "enc_generic", (16, 2): "enc_generic"}


def drive(sz, oracle, no_fast, codec, D, data, chunk_len, family, tag):
    """integers as float32 with scale 1 and offset 0 are exact: the container is the ORACLE's streams of the integers"""
    import torch
    esz = data.dtype.itemsize
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device="cuda:0")
    src = torch.from_numpy(data.astype(np.float32)).cuda()
    nchunks = -(-data.size // chunk_len)
    for fam in (0, 1):
        no_fast(fam)
        enc, dense = ask(cd, nchunks, data.size, qm.F32, fam)
        assert enc == (family if not fam else "enc_generic"), (tag, enc)
        if fam and family == "enc_generic":
            continue
        with ran(only=[enc, dense], **{enc: 1, dense: 1}):
            got = float_dense(cd, src, qm.F32, None, None, False, bool(fam))      # (on integers floor and rint agree)
        check_streams(oracle, codec, data, chunk_len, D, got["data"], got["offsets"], got["sizes"], tag)
        assert (got["rets"] == np.array([int(s) // esz for s in got["sizes"]])).all(), tag
    no_fast(0)


@pytest.mark.parametrize("w,D,nblocks,r", RLE_SHAPES, ids=[f"u{w}x{D}" for w, D, _, _ in RLE_SHAPES])
def test_the_rle_drive_through_the_converting_loads(sz, oracle, no_fast, w, D, nblocks, r):
    """tests/rle_drive.py's batches: run ends in both slots, 0x7f / 0x7fff runs, runs at chunk starts and ends"""
    for codec in ("delta", "xff"):
        for kind in rd.KINDS:
            data, chunk_len, _ = rle_batch_of(codec, w, D, kind, NCHUNKS, nblocks, r)
            assert chunk_len % D == 0
            drive(sz, oracle, no_fast, codec, D, data, chunk_len, RLE_FAMILY[(w, D)], f"rle u{w}x{D} {codec} {kind}")


FIRE_SHAPES = {(8, 8): (7, "enc_pair"), (8, 6): (5, "enc_pair"), (8, 32): (6, "enc_pair"), (8, 80): (5, "enc_split"), (8, 96): (5, "enc_wide"), (8, 5): (6, "enc_generic"),
               (8, 1): (7, "enc_generic"), (16, 2): (5, "enc_generic")}


@pytest.mark.parametrize("w,D", list(FIRE_SHAPES), ids=[f"u{w}x{D}" for w, D in FIRE_SHAPES])
def test_the_fire_drive_through_the_converting_loads(sz, oracle, no_fast, w, D):
    """tests/fire_drive.py's batches: FIRE counters through their int16 wrap, runs at frozen extreme coefficients"""
    nchunks, family = FIRE_SHAPES[(w, D)]
    data, chunk_len = fire_batch_of(w, D, nchunks)
    drive(sz, oracle, no_fast, "xff", D, data, chunk_len, family, f"fire u{w}x{D}")


# ------------------------------------------------------------------ the headline shape, a misaligned source

def test_headline_shape_is_one_launch(sz, no_fast):
    """uint16 x 8, 5 120-element chunks, 64 x 3 chunks: the dense call is enc_pair = 1, dense_fused = 1 and nothing else moved; the slots
    call followed by compact gives the same container"""
    import torch
    from sprintz_amd import _lib
    esz, D, chunk_len, nchunks = 2, 8, 5120, 192
    n = nchunks * chunk_len
    rng = np.random.default_rng(7)
    inv, off = qm.column_params(D)
    x = make_values(rng, "walk", n, esz, D, chunk_len, inv, off)
    cd = sz.ChunkedCodec("xff", esz, D, chunk_len, device="cuda:0")
    no_fast(0)
    for fmt in qm.FORMATS:
        bits = qm.source_bits(x, fmt)
        q = qm.compress_floats(qm.source_values(bits, fmt), chunk_len, D, 16, inv, off)
        want = int_dense(cd, q)
        src, _owner = to_tensor(bits, fmt)
        assert ask(cd, nchunks, n, fmt) == ("enc_pair", "dense_fused")
        with ran(only=["enc_pair", "dense_fused"], enc_pair=1, dense_fused=1):
            got = float_dense(cd, src, fmt, inv, off, False, False)
        assert_same(sz, cd, got, want, q, ("headline", qm.NAMES[fmt]))
        # the slots call, then compact
        ws = cd.workspace(nchunks)
        i, o = torch.from_numpy(inv).cuda(), torch.from_numpy(off).cuda()
        with ran(only=["enc_pair"], enc_pair=1):
            _lib.check(_lib.compress_batch_float(1, esz, src.data_ptr(), fmt, i.data_ptr(), o.data_ptr(), 0, n, chunk_len, D, ws["slots"].data_ptr(), cd.slot_stride,
                                                 ws["sizes"].data_ptr(), ws["rets"].data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        with ran(only=["dense_compact"], dense_compact=1):
            dense, offsets = cd.compact(ws, nchunks)
        total = int(offsets[-1].item())
        assert np.array_equal(offsets.cpu().numpy(), want["offsets"]) and np.array_equal(dense[:total].cpu().numpy(), want["data"])
        assert np.array_equal(ws["sizes"].cpu().numpy(), want["sizes"]) and np.array_equal(ws["rets"].cpu().numpy(), want["rets"])


@pytest.mark.parametrize("esz,D", [(2, 8), (1, 80)])
def test_misaligned_source_runs_on_the_generic_kernel(sz, no_fast, esz, D):
    """a float32 source shifted by one element (d_src % 16 == 4): enc_generic, the same bytes"""
    chunk_len = named_chunk_len(esz, D)
    n = 5 * chunk_len - D // 2
    rng = np.random.default_rng(D)
    inv, off = qm.column_params(D)
    x = make_values(rng, "walk", n, esz, D, chunk_len, inv, off)
    cd = sz.ChunkedCodec("delta", esz, D, chunk_len, device="cuda:0")
    bits = qm.source_bits(x, qm.F32)
    q = qm.compress_floats(bits, chunk_len, D, 8 * esz, inv, off)
    want = int_dense(cd, q)
    no_fast(0)
    for shift, lo in ((0, 0), (1, 4), (4, 0), (3, 12)):
        src, _owner = to_tensor(bits, qm.F32, shift)
        assert src.data_ptr() % 16 == lo
        enc, dense = ask(cd, 5, n, qm.F32, 0, lo)
        assert enc == (FAMILY[(esz, D)] if lo == 0 else "enc_generic")
        with ran(only=[enc, dense], **{enc: 1, dense: 1}):
            got = float_dense(cd, src, qm.F32, inv, off, False, False)
        assert_same(sz, cd, got, want, q, ("misaligned", esz, D, shift))


# ------------------------------------------------------------------ Python

def test_compress_floats_python(sz):
    import torch
    import float_model as fm
    from sprintz_amd import datasets, rowops
    rng = np.random.default_rng(5)
    esz, D, rows = 2, 8, 640 * 5 + 100
    m = rng.normal(size=(rows, D)) * rng.uniform(0.1, 50.0, size=D) + rng.uniform(-20, 20, size=D)
    m[:, 3] = 1.5                                                                   # a constant column
    scale, offset = datasets.dequantize_params(m, np.uint16)
    chunk_len = 640 * D
    cd = sz.ChunkedCodec("xff", esz, D, chunk_len, device="cuda:0")
    inv, off = (t.numpy() for t in rowops.quant_params(scale, offset, D, torch.device("cpu")))
    for fmt, dt in ((qm.F32, torch.float32), (qm.F16, torch.float16), (qm.BF16, torch.bfloat16)):
        x = torch.from_numpy(m).to(dt).cuda()                                       # [rows, D]
        bits = x.cpu().view(torch.int32 if fmt == qm.F32 else torch.int16).numpy().reshape(-1)
        v = qm.source_values(bits.view(np.float32) if fmt == qm.F32 else bits.view(np.uint16), fmt)
        for signed, rounding in ((False, "nearest"), (False, "floor"), (True, "nearest")):
            q = qm.compress_floats(v, chunk_len, D, 16, inv, off, signed, rounding == "floor")
            batch = cd.compress_floats(x, scale, offset, signed=signed, rounding=rounding)
            assert batch.nchunks == -(-q.size // chunk_len) and batch.total_len == q.size and batch.ndims == D
            assert np.array_equal(cd.decompress(batch).cpu().numpy().view(np.uint16)[:q.size], q), (qm.NAMES[fmt], signed, rounding)
            want = cd.compress(torch.from_numpy(q.view(np.int16).copy()).cuda().view(torch.uint16))
            assert same_batch(batch, want), (qm.NAMES[fmt], signed, rounding)
            # the round trip through float_rows is the two models composed, as bits
            back = cd.float_rows(batch, dtype=dt, scale=scale, offset=offset, signed=signed)
            view = torch.int32 if fmt == qm.F32 else torch.int16
            assert np.array_equal(back.view(view).cpu().numpy().view(fm.BITS_DTYPE[fmt]).reshape(-1), fm.float_rows(q, chunk_len, D, scale, offset, signed, fmt))
        # tensors on the device as parameters; a non-contiguous source is made contiguous
        b2 = cd.compress_floats(x, torch.from_numpy(scale).cuda(), list(offset))
        b1 = cd.compress_floats(x, scale, offset)
        assert same_batch(b1, b2)
        wide = torch.zeros(rows, 2 * D, dtype=dt, device="cuda")
        wide[:, :D] = x
        assert not wide[:, :D].is_contiguous()
        b3 = cd.compress_floats(wide[:, :D], scale, offset)
        assert same_batch(b1, b3)
    # scale=None, offset=None: the values themselves, rounded and clamped
    ints = rng.integers(-5, 70000, rows * D).astype(np.float32) + rng.choice([0.0, 0.5, 0.25], rows * D).astype(np.float32)
    bn = cd.compress_floats(torch.from_numpy(ints).cuda())
    assert np.array_equal(cd.decompress(bn).cpu().numpy().view(np.uint16)[:ints.size], qm.compress_floats(ints, chunk_len, D, 16))
    empty = cd.compress_floats(torch.empty(0, dtype=torch.float32, device="cuda"))
    assert empty.nchunks == 0 and empty.total_len == 0 and int(empty.offsets[-1].item()) == 0
    # the round trip on the values: within half a step (nearest), up to float32 rounding
    back = cd.float_rows(cd.compress_floats(torch.from_numpy(m.astype(np.float32)).cuda(), scale, offset), scale=scale, offset=offset).cpu().numpy().astype(np.float64)
    span = m.max(axis=0) - m.min(axis=0)
    slack = 16 * 2.0 ** -24 * (np.abs(m).max(axis=0) + np.maximum(1, span))
    assert np.all(np.abs(back - m) <= 0.5 * scale.astype(np.float64) + slack)
    # refusals
    x32 = torch.from_numpy(m.astype(np.float32)).cuda()
    for src, kw in ((x32.double(), {}), (x32.to(torch.int16), {}), (x32.cpu(), {}), (x32, dict(scale=0.0)), (x32, dict(scale=float("inf"))), (x32, dict(offset=[float("nan")] * D)),
                    (x32, dict(scale=[1.0] * (D + 1))), (x32, dict(rounding="up")), (m, {})):
        with pytest.raises(ValueError):
            cd.compress_floats(src, **kw)
    with pytest.raises(ValueError):
        sz.ChunkedCodec("xff", 2, 8, chunk_len, device="cuda:0", align=8).compress_floats(x32)
    with pytest.raises(ValueError):
        sz.ChunkedCodec("xff", 2, 8, 8 * 640 + 3, device="cuda:0").compress_floats(x32)        # chunk_len % ndims != 0
    with pytest.raises(sz.SprintzError, match="compress_batch_float_dense"):
        sz.ChunkedCodec("delta_norle", 2, 8, chunk_len, device="cuda:0").compress_floats(x32)
