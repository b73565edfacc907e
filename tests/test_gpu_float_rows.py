"""GPU tests (-m gpu) of float rows (sprintz_mi355x_float_rows, ChunkedCodec.float_rows): a compressed batch decoded straight into scaled
float32 / float16 / bfloat16.

The expected value is always the numpy model (tests/float_model.py) on the ORIGINAL input, compared as bits; column d takes parameter
pair d % 8 of the model's list, so a value converted with another column's parameters shows.  Every launch asserts its kernel family
(tests/dispatch.py), as the planner probe (tests/plan_probe.cpp) gives it for the shape."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import float_model as fm
import planner
from drive_tables import ROWOP_CASES, ROWOP_IDS, rowop_batch
from fixtures import chunks_per_group, no_fast, sz  # noqa: F401  (fixtures)
from rowdata import FLOAT_FAST_SHAPES as FAST_SHAPES, GENERIC_SHAPES, chunk_len_for, gen_data, make_batch, parity_cases
from streams import GENERIC, OLD, fire_batch_of as batch_of, fire_oracle_batch as oracle_batch, options
from dispatch import ran
from harness import DTYPES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PAD = 4096                                             # sentinel elements behind every output
SENT = {2: 0x5A5A, 4: 0x5A5A5A5A}                       # by output element size
CODEC_ID = {"delta": 0, "xff": 1}


@pytest.fixture(scope="module")
def plan():
    """the planner on a host compiler: -> f(**fields) -> the family's name"""
    planner.available(required=True)

    def ask(**fields):
        got = planner.ask("decode", q=planner.QUERY["float"], **fields)
        assert got.get("family") in ("dec_fast", "dec_generic"), got
        return got["family"]
    return ask


def run_float(batch, codec, esz, D, chunk_len, fmt, signed=False, scale=None, offset=None, general=False, shift=0):
    """the C entry point on a sentinel-filled output of `shift` elements, nchunks * chunk_len elements and PAD more
    -> (the whole buffer as bits, rets [nchunks + 1] with a sentinel behind)"""
    import torch
    from sprintz_amd import _lib
    n = batch.nchunks
    osz = fm.OUT_BYTES[fmt]
    buf = torch.full((shift + n * chunk_len + PAD,), SENT[osz], dtype=torch.int16 if osz == 2 else torch.int32, device="cuda")
    rets = torch.full((n + 1,), -77, dtype=torch.int64, device="cuda")
    s = None if scale is None else torch.from_numpy(np.ascontiguousarray(scale, np.float32)).cuda()
    o = None if offset is None else torch.from_numpy(np.ascontiguousarray(offset, np.float32)).cuda()
    flags = (_lib.QUERY_GENERAL_LAYOUT if general else 0) | (_lib.FLOAT_SIGNED if signed else 0)
    _lib.check(_lib.float_rows(CODEC_ID[codec], esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, chunk_len, D, fmt,
                               None if s is None else s.data_ptr(), None if o is None else o.data_ptr(), flags,
                               buf.data_ptr() + shift * osz, rets.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(fm.BITS_DTYPE[fmt]), rets.cpu().numpy()


def assert_float(h, rets, x, chunk_len, nchunks, want, fmt, shift, msg, bad=()):
    """the buffer against the model's bits `want` of the batch's x.size elements: the chunks outside `bad` are the model's, and nothing is
    written in front, behind, or past the short last chunk's count; rets are the chunks' element counts (outside `bad`)"""
    sent = SENT[fm.OUT_BYTES[fmt]]
    n, ne = x.size, nchunks * chunk_len
    assert np.all(h[:shift] == sent), ("written in front",) + msg
    assert np.all(h[shift + ne:] == sent) and h.size == shift + ne + PAD, ("written behind",) + msg
    body = h[shift:shift + ne]
    assert np.all(body[n:] == sent), ("written past the last chunk's count",) + msg
    keep = np.ones(n, bool)
    for c in bad:
        keep[c * chunk_len:(c + 1) * chunk_len] = False
    ne_ = body[:n][keep] != want[keep]
    assert not ne_.any(), (int(ne_.sum()), "of", int(keep.sum()), "elements differ; first at", int(np.flatnonzero(keep)[np.flatnonzero(ne_)[0]])) + msg
    lens = [min(chunk_len, n - c * chunk_len) for c in range(nchunks)]
    assert all(rets[c] == lens[c] for c in range(nchunks) if c not in bad) and all(rets[c] < 0 for c in bad) and rets[nchunks] == -77, ("rets", rets.tolist()) + msg


def rotate(key, k):
    return zlib.crc32(key.encode()) % k


# ------------------------------------------------------------------ parity

def named_chunk_len(esz, D):
    """about 8 KB of whole groups of 16 rows -- at least four, so that decode_fast.h takes the chunk -- and a verbatim tail of 3 rows"""
    return D * (16 * max(4, 8192 // (16 * D * esz)) + 3)


def named_cases():
    return [(codec, esz, D) for codec in ("delta", "xff") for esz, D in FAST_SHAPES + GENERIC_SHAPES]


@pytest.mark.parametrize("codec,esz,D", named_cases())
def test_float_rows_parity_named_shapes(sz, oracle, no_fast, plan, codec, esz, D):
    """the sixteen shapes named for the planner probe: both families, signed and unsigned, all three formats"""
    rng = np.random.default_rng(zlib.crc32(f"float{codec}{esz}{D}".encode()))
    chunk_len = named_chunk_len(esz, D)
    nchunks = 5 + D % 4
    n = nchunks * chunk_len - (chunk_len // (3 * D)) * D - D // 2        # a short last chunk that ends mid-row (D > 1)
    x = gen_data(("walk", "uniform", "sparse")[rotate(f"{codec}{esz}{D}", 3)], rng, n, esz, D)
    general = bool(rotate(f"g{codec}{esz}{D}", 2))
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, general)
    scale, offset = fm.column_params(D)
    for fam in (0, 1):
        no_fast(fam)
        for fmt in fm.FORMATS:
            family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], out_esz=fm.OUT_BYTES[fmt], general=general, no_fast=fam)
            assert family == ("dec_fast" if (esz, D) in FAST_SHAPES and not fam else "dec_generic")
            for signed in (False, True):
                with ran(only=[family], **{family: 1}):
                    h, rets = run_float(batch, codec, esz, D, chunk_len, fmt, signed, scale, offset, general)
                assert_float(h, rets, x, chunk_len, nchunks, fm.float_rows(x, chunk_len, D, scale, offset, signed, fmt), fmt, 0,
                             (codec, esz, D, family, fm.NAMES[fmt], signed, general))


@pytest.mark.parametrize("codec,esz,D,shape,data,general", [c for c in parity_cases() if chunk_len_for(c[3], c[2]) % c[2] == 0])
def test_float_rows_parity(sz, oracle, no_fast, plan, codec, esz, D, shape, data, general):
    """the whole-row cases of the windowed query's parity: both families, signed and unsigned, one format a case"""
    key = f"{codec}{esz}{D}{shape}{data}{general}"
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    chunk_len = chunk_len_for(shape, D)
    nchunks = 5 + D % 4
    n = nchunks * chunk_len - chunk_len // 3 - 1          # every batch ends in a short last chunk
    x = gen_data(data, rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, general)
    scale, offset = fm.column_params(D)
    fmt = fm.FORMATS[rotate(key, 3)]
    for fam in (0, 1):
        no_fast(fam)
        family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], out_esz=fm.OUT_BYTES[fmt], general=general, no_fast=fam)
        for signed in (False, True):
            with ran(only=[family], **{family: 1}):
                h, rets = run_float(batch, codec, esz, D, chunk_len, fmt, signed, scale, offset, general)
            assert_float(h, rets, x, chunk_len, nchunks, fm.float_rows(x, chunk_len, D, scale, offset, signed, fmt), fmt, 0,
                         (codec, esz, D, shape, data, general, family, fm.NAMES[fmt], signed))


# ------------------------------------------------------------------ the edges of the buffer

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 16), ("xff", 2, 128), ("delta", 2, 5)])
def test_float_rows_edges_of_the_buffer(sz, oracle, plan, codec, esz, D):
    """a chunk with a verbatim tail (chunk_len is no multiple of 8 * ndims), a last chunk that ends mid-row; the output shifted by 16
    elements (still on the 16-byte grid: decode_fast.h where the shape allows) and by one (the generic kernel)"""
    rng = np.random.default_rng(D)
    chunk_len = D * (16 * max(4, 8192 // (16 * D * esz)) + 11)
    assert chunk_len % (8 * D) != 0
    nchunks = 6
    n = (nchunks - 1) * chunk_len + D * 37 + max(1, D // 2)
    assert n % D != 0 or D == 1
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    scale, offset = fm.column_params(D)
    seen = set()
    for fmt in fm.FORMATS:
        want = fm.float_rows(x, chunk_len, D, scale, offset, False, fmt)
        for shift in (0, 16, 1):
            family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], out_esz=fm.OUT_BYTES[fmt], out_lo=(shift * fm.OUT_BYTES[fmt]) % 16)
            assert family == ("dec_fast" if (D * esz) % 16 == 0 and shift != 1 else "dec_generic")
            seen.add(family)
            with ran(only=[family], **{family: 1}):
                h, rets = run_float(batch, codec, esz, D, chunk_len, fmt, False, scale, offset, False, shift)
            assert_float(h, rets, x, chunk_len, nchunks, want, fmt, shift, (codec, esz, D, fm.NAMES[fmt], shift, family))
    assert "dec_generic" in seen


# ------------------------------------------------------------------ identity

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 80), ("xff", 1, 3)])
def test_float_rows_identity(sz, oracle, codec, esz, D):
    """float32 with NULL scale and offset is decompress(batch).to(float32), exactly; explicit ones and zeros give the same bits"""
    import torch
    rng = np.random.default_rng(17 * D)
    chunk_len = D * (16 * max(4, 8192 // (16 * D * esz)) + 5)
    n = 6 * chunk_len - 2 * D
    x = gen_data("uniform", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    plain = cd.decompress(batch)
    assert np.array_equal(plain.cpu().numpy().view(DTYPES[esz]), x)
    want = plain.to(torch.int32).to(torch.float32) if esz == 2 else plain.to(torch.float32)
    for fmt, dt in ((fm.F32, torch.float32), (fm.F16, torch.float16), (fm.BF16, torch.bfloat16)):
        null = cd.float_rows(batch, dtype=dt)
        ones = cd.float_rows(batch, dtype=dt, scale=torch.ones(D, device="cuda"), offset=np.zeros(D))
        assert null.dtype == dt and null.shape == (n // D, D)
        view = torch.int32 if fmt == fm.F32 else torch.int16
        assert torch.equal(null.view(view), ones.view(view)), (codec, esz, D, fm.NAMES[fmt])
        assert torch.equal(null.view(view).reshape(-1), want.to(dt).view(view)), (codec, esz, D, fm.NAMES[fmt])
        assert np.array_equal(null.view(view).reshape(-1).cpu().numpy().view(fm.BITS_DTYPE[fmt]), fm.float_rows(x, chunk_len, D, fmt=fmt))


# ------------------------------------------------------------------ the drives

def float_legs(w, D):
    """(options, chunks_per_group, family): decode_fast.h at one and at three chunks a lane group where the rows are whole 16-byte pieces,
    then the generic kernel"""
    fast = (D * w // 8) % 16 == 0
    return ([(OLD, 1, "dec_fast"), (OLD, 3, "dec_fast")] if fast else []) + [(GENERIC if fast else OLD, 1, "dec_generic")]


def drive(batch, data, codec, w, D, chunk_len, nchunks, chunks_per_group, key):
    scale, offset = fm.column_params(D)
    for j, (fmt, signed) in enumerate(((fm.FORMATS[rotate(key, 3)], False), (fm.FORMATS[(rotate(key, 3) + 1) % 3], True))):
        want = fm.float_rows(data, chunk_len, D, scale, offset, signed, fmt)
        for opts, cpg, family in float_legs(w, D):
            with options(**opts):
                chunks_per_group(cpg)
                with ran(only=[family], **{family: 1}):
                    h, rets = run_float(batch, codec, w // 8, D, chunk_len, fmt, signed, scale, offset)
            assert_float(h, rets, data, chunk_len, nchunks, want, fmt, 0, (key, fm.NAMES[fmt], signed, family, cpg))


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_float_rows_over_runs(sz, oracle, chunks_per_group, codec, w, D, kind):
    """tests/rle_drive.py's batches: runs at chunk starts and ends, of 1 .. 16 blocks and maximal ones, closed inside a step -- the held
    slots and the immediate run stores of decode_fast.h, at one and at three chunks a lane group"""
    cd, batch, data, chunk_len, _ = rowop_batch(sz, oracle, codec, w, D, kind)
    drive(batch, data, codec, w, D, chunk_len, batch.nchunks, chunks_per_group, f"{codec}{w}{D}{kind}")


FIRE_SHAPES = {(8, 8): 7, (16, 1): 5, (8, 16): 4}        # (w, D): chunks -- the row operations' two shapes, and one whose rows are whole pieces


@pytest.mark.parametrize("w,D", list(FIRE_SHAPES), ids=[f"u{w}x{D}" for w, D in FIRE_SHAPES])
def test_float_rows_on_the_fire_drive(sz, oracle, chunks_per_group, w, D):
    """tests/fire_drive.py's batches: FIRE counters through their int16 wrap, runs replayed at frozen extreme coefficients"""
    nchunks = FIRE_SHAPES[(w, D)]
    data, chunk_len = batch_of(w, D, nchunks)
    batch = oracle_batch(sz, oracle, D, data, chunk_len)
    drive(batch, data, "xff", w, D, chunk_len, nchunks, chunks_per_group, f"fire{w}{D}")


# ------------------------------------------------------------------ damage

def damaged_batch(sz, batch, cut, flip):
    """the container with chunk `cut`'s stream 5 bytes short (the streams packed densely again) and one bit of chunk `flip`'s header flipped"""
    import torch
    n = batch.nchunks
    comp, offs, sizes = batch.data.cpu().numpy(), batch.offsets.cpu().numpy(), batch.sizes.cpu().numpy()
    parts = [comp[offs[c]:offs[c] + sizes[c] - (5 if c == cut else 0)].copy() for c in range(n)]
    parts[flip][6] ^= 0x04                                                         # the header's ndims field
    toffs = np.zeros(n + 1, np.int64)
    toffs[1:] = np.cumsum([p.size for p in parts])
    return sz.CompressedBatch(torch.from_numpy(np.concatenate(parts + [np.zeros(sz._lib.READ_SLACK, np.uint8)])).cuda(), torch.from_numpy(toffs).cuda(),
                              torch.tensor([p.size for p in parts], dtype=torch.int32).cuda(), n, batch.total_len, batch.chunk_len, batch.ndims)


@pytest.mark.parametrize("codec,esz,D,fam", [("xff", 2, 8, 0), ("delta", 1, 32, 0), ("xff", 2, 8, 1), ("delta", 2, 12, 0)])
def test_float_rows_damaged_chunks(sz, oracle, no_fast, chunks_per_group, codec, esz, D, fam):
    """one truncated and one bit-flipped stream, inside lane groups of three: d_rets is decompress_batch's, every other chunk is right,
    the padding is intact, and check=True names the first damaged chunk"""
    import torch
    rng = np.random.default_rng(3 * D + fam)
    chunk_len = D * 16 * max(4, 8192 // (16 * D * esz)) + 3 * D
    nchunks, cut, flip = 8, 2, 4
    n = nchunks * chunk_len - 5 * D
    x = gen_data("walk", rng, n, esz, D)
    cd, good = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    batch = damaged_batch(sz, good, cut, flip)
    scale, offset = fm.column_params(D)
    family = "dec_fast" if (D * esz) % 16 == 0 and not fam else "dec_generic"
    with options(**OLD):
        no_fast(fam)
        chunks_per_group(3)
        plain_rets = torch.full((nchunks,), -77, dtype=torch.int64, device="cuda")
        cd.decompress(batch, rets=plain_rets)
        plain_rets = plain_rets.cpu().numpy()
        assert plain_rets[cut] < 0 and plain_rets[flip] < 0 and np.all(np.delete(plain_rets, [cut, flip]) > 0)
        for fmt in fm.FORMATS:
            with ran(only=[family], **{family: 1}):
                h, rets = run_float(batch, codec, esz, D, chunk_len, fmt, True, scale, offset)
            assert np.array_equal(rets[:nchunks], plain_rets), (rets.tolist(), plain_rets.tolist())
            assert_float(h, rets, x, chunk_len, nchunks, fm.float_rows(x, chunk_len, D, scale, offset, True, fmt), fmt, 0, (codec, esz, D, family, fm.NAMES[fmt]),
                         bad=(cut, flip))
        with pytest.raises(sz.SprintzError, match=f"float_rows: chunk {cut} "):
            cd.float_rows(batch, scale=scale, offset=offset)
        got = cd.float_rows(batch, scale=scale, offset=offset, check=False)
        assert got.shape == (n // D, D)
        cd.float_rows(good, scale=scale, offset=offset)                             # undamaged: no error
    chunks_per_group(1)


# ------------------------------------------------------------------ past 4 GiB

def test_float_rows_output_past_4_gib(sz):
    """uint8 x 16 decoded to more than 4 GiB of float32 on decode_fast.h: the store descriptor's base is 64-bit a wave.  Compared on the
    device with decompress().to(float32) * 0.5 - 3 (exact in float32) over the first chunk, the last one and those on both sides of the
    4 GiB line"""
    import torch
    D, chunk_len = 16, 10240
    nchunks = 105000
    n = nchunks * chunk_len - 7 * D
    assert n * 4 > (1 << 32) + (1 << 20)
    r = torch.arange(n // D, device="cuda", dtype=torch.int32)
    x = ((r[:, None] * 3 + (r[:, None] >> 9) * 17 + torch.arange(D, device="cuda", dtype=torch.int32) * 29) & 0xFF).to(torch.uint8).reshape(-1)
    del r
    cd = sz.ChunkedCodec("xff", 1, D, chunk_len, device="cuda:0")
    batch = cd.compress(x)
    assert batch.nchunks == nchunks
    with ran(only=["dec_fast"], dec_fast=1):
        out = cd.float_rows(batch, scale=0.5, offset=-3.0)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == (n // D, D)
    flat = out.reshape(-1)
    line = (1 << 32) // 4 // chunk_len                                              # the chunk the 4 GiB line falls in
    assert 0 < line < nchunks - 2
    for c in (0, line - 1, line, line + 1, nchunks - 1):
        lo, hi = c * chunk_len, min((c + 1) * chunk_len, n)
        want = x[lo:hi].to(torch.float32) * 0.5 - 3.0
        assert torch.equal(flat[lo:hi], want), c
    plain = cd.decompress(batch)
    assert torch.equal(plain[line * chunk_len:(line + 1) * chunk_len], x[line * chunk_len:(line + 1) * chunk_len])


# ------------------------------------------------------------------ Python

def test_float_rows_python(sz, oracle):
    import torch
    from sprintz_amd import datasets
    rng = np.random.default_rng(5)
    esz, D, rows = 2, 8, 640 * 5 + 100
    m = rng.normal(size=(rows, D)) * rng.uniform(0.1, 50.0, size=D) + rng.uniform(-20, 20, size=D)
    m[:, 3] = 1.5                                                                   # a constant column
    q = datasets.quantize(m, np.uint16)
    scale, offset = datasets.dequantize_params(m, np.uint16)
    chunk_len = 640 * D
    cd = sz.ChunkedCodec("xff", esz, D, chunk_len, device="cuda:0")
    batch = cd.compress(torch.from_numpy(q.view(np.int16).reshape(-1)).cuda().view(torch.uint16))
    x = q.reshape(-1)
    for fmt, dt in ((fm.F32, torch.float32), (fm.F16, torch.float16), (fm.BF16, torch.bfloat16)):
        view = torch.int32 if fmt == fm.F32 else torch.int16
        want = fm.float_rows(x, chunk_len, D, scale, offset, False, fmt)
        got = cd.float_rows(batch, dtype=dt, scale=scale, offset=offset)
        assert got.dtype == dt and got.shape == (rows, D) and got.device.type == "cuda"
        assert np.array_equal(got.view(view).cpu().numpy().view(fm.BITS_DTYPE[fmt]).reshape(-1), want)
        # a tensor scale on the device, a sequence offset, out= and rets=
        out = torch.full((batch.nchunks * chunk_len + 64,), 7.0, dtype=dt, device="cuda")
        rets = torch.full((batch.nchunks,), -77, dtype=torch.int64, device="cuda")
        got2 = cd.float_rows(batch, dtype=dt, scale=torch.from_numpy(scale).cuda(), offset=list(offset), out=out, rets=rets)
        assert got2.data_ptr() == out.data_ptr() and torch.equal(got2.view(view), got.view(view))
        assert torch.all(out[x.size:] == 7.0) and rets.tolist() == [chunk_len] * (batch.nchunks - 1) + [x.size - (batch.nchunks - 1) * chunk_len]
        # signed, a scalar scale
        sg = cd.float_rows(batch, dtype=dt, scale=0.25, signed=True)
        assert np.array_equal(sg.view(view).cpu().numpy().view(fm.BITS_DTYPE[fmt]).reshape(-1), fm.float_rows(x, chunk_len, D, np.full(D, 0.25), None, True, fmt))
    # the round trip: within one quantisation step below the value (quantize truncates), up to float32 rounding
    back = cd.float_rows(batch, scale=scale, offset=offset).cpu().numpy().astype(np.float64)
    span = m.max(axis=0) - m.min(axis=0)
    slack = 8 * 2.0 ** -24 * (np.abs(m).max(axis=0) + np.maximum(1, span))
    err = back - m
    assert np.all(err <= slack) and np.all(err >= -(scale.astype(np.float64) + slack))
    # refusals
    for kw in (dict(dtype=torch.float64), dict(dtype=torch.int16), dict(scale=float("inf")), dict(offset=[float("nan")] * D), dict(scale=[1.0] * (D + 1)),
               dict(out=torch.empty(8, device="cuda")), dict(out=torch.empty(batch.nchunks * chunk_len, dtype=torch.float16, device="cuda")),
               dict(out=torch.empty(batch.nchunks * chunk_len, 2, device="cuda")[:, 0])):
        with pytest.raises(ValueError):
            cd.float_rows(batch, **kw)
    with pytest.raises(ValueError):
        sz.ChunkedCodec("xff", 2, 8, 8 * 640 + 3, device="cuda:0").float_rows(batch)      # chunk_len % ndims != 0
