"""GPU tests (-m gpu) of gather rows (sprintz_mi355x_gather_rows, ChunkedCodec.gather_rows / read_rows): N row ranges of a
compressed batch decoded in one launch by the gather mode of decode_fast.h and of decode_kernel.h.  The expected samples
are always rows of the ORIGINAL input -- decode is lossless and pinned elsewhere.  Both families deliver the same rows, so wherever a
case names its family -- `fam` (SPRINTZ_OPT_NO_FAST), a shape marked decode_fast -- the call also asserts it from the dispatch counters."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

import gather_model as gm
from dispatch import ran
from harness import DTYPES, gen_sparse
from fixtures import no_fast, sz  # noqa: F401  (fixtures)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

pytestmark = pytest.mark.gpu

NDIMS = [1, 2, 3, 4, 5, 8, 16, 33, 80, 128, 200, 256, 300, 512]
SHAPES = ["r16", "tail", "nogroups"]
DATA = ["walk", "uniform", "constant", "sparse"]
ROWS = ["1", "7", "8", "R-1", "R", "R+1", "3R+5"]


def gathers_on(fam, fast_shape=None):
    """the dispatch assertion around ONE gather_rows call: fam 1 (SPRINTZ_OPT_NO_FAST) -> the generic kernel whatever the shape; fam 0 ->
    decode_fast.h's gather mode where the shape is its (general layout, at most 256 columns, rows of whole 16-byte pieces, chunks of at
    least half its ring, a 16-byte aligned output), the generic kernel where it is not; fast_shape None: the case does not say"""
    if fam == 0 and fast_shape is None:
        return ran(one_of=["gather_fast", "gather_generic"], only=["gather_fast", "gather_generic"])
    k = "gather_fast" if fam == 0 and fast_shape else "gather_generic"
    return ran(only=[k], **{k: 1})


def fast_ring_bytes(esz, D):
    """LDS one lane group of decode_fast.h's gather mode holds (decode_fast_lds_bytes): the read-ahead ring -- whole units of 16 bytes a lane
    and column, at least twice the largest stream group (header + two packed blocks) and one unit more -- its apron and one block of staging.
    The lanes: the next power of two up to 64, then 2 / 4 columns a lane."""
    dp, cpl = 4, 1
    while dp < D and dp < 64:
        dp *= 2
    while dp * cpl < D:
        cpl *= 2
    unit, dcap = dp * 16 * cpl, dp * cpl
    cg = (2 * dcap * (3 if esz == 1 else 4) + 7) // 8 + 2 * 8 * dcap * esz + 4
    ring = ((2 * (cg + 24) + 3 + unit - 1) // unit + 1) * unit
    return ring + ((cg + 24 + 8 + 15) & ~15) + ((8 * D * esz + 15) & ~15) + 16


def fast_shape_of(esz, D, chunk_len):
    """the shapes sprintz_mi355x_gather_rows serves from decode_fast.h (given a 16-byte aligned output and a container below 4 GB): the general
    layout, at most 256 columns, rows of whole 16-byte pieces, chunks of at least half the ring"""
    lowdim = D <= 4 if esz == 1 else D <= 2
    return not lowdim and D <= 256 and (D * esz) % 16 == 0 and 2 * chunk_len * esz >= fast_ring_bytes(esz, D)


def rows_per_chunk(shape, D):
    r16 = 16 * max(2, 2048 // (16 * D))
    if shape == "r16":                                    # whole groups of 16 rows
        return r16
    if shape == "tail":                                   # a verbatim tail of 1 .. 15 rows
        return r16 + 1 + D % 15
    return 13                                             # shorter than one group


def rows_for(kind, R):
    return {"1": 1, "7": 7, "8": 8, "R-1": max(1, R - 1), "R": R, "R+1": R + 1, "3R+5": 3 * R + 5}[kind]


def gen_rows(kind, rng, total_rows, esz, D):
    """-> [total_rows, D]"""
    top = 1 << (8 * esz)
    n = total_rows * D
    if kind == "uniform":
        x = rng.integers(0, top, n).astype(DTYPES[esz])
    elif kind == "constant":
        x = np.full(n, 0xA5 if esz == 1 else 0x1234, DTYPES[esz])
    elif kind == "sparse":                                # long zero runs
        x = gen_sparse(rng, n, esz, 0.02)
    else:                                                 # walk of +-8 with flat spans of 50 rows: runs of both codecs
        steps = rng.integers(-8, 9, size=(total_rows, D), dtype=np.int64)
        steps[(np.arange(total_rows) // 50) % 3 == 1] = 0
        x = np.mod(np.cumsum(steps, axis=0) + rng.integers(0, top, size=(1, D)), top).astype(DTYPES[esz])
    return np.ascontiguousarray(x.reshape(total_rows, D))


def compress(sz, codec, esz, D, chunk_len, x):
    import torch
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device="cuda:0")
    return cd, cd.compress(torch.from_numpy(x.view(np.int8 if esz == 1 else np.int16)).cuda().view(cd.dtype))


def start_vector(rng, rows, R, total):
    """0, a chunk edge and its neighbours, a start inside a run (rows 50 .. 99 of the walk are flat; constant and sparse data
    are runs nearly everywhere), a range that ends on the first row of a chunk's verbatim tail region (its last 15 rows hold
    the tail of every shape), the last `rows` rows of the batch, a duplicate, two overlapping ranges -- shuffled"""
    nfull = total // R
    c = min(2, max(1, nfull - 1))
    cand = [0, c * R, c * R - 1, c * R + 1, 60, 60 + rows // 2, total - rows, 0]
    for back in (1, 8, 15):                                # last needed row: 1 / 8 / 15 rows before a chunk's end
        cand.append(nfull * R - back - rows + 1)
    cand.append((nfull - 1) * R + 3)                       # into the last full chunk, maybe on into the short one
    s = np.array([v for v in cand if 0 <= v <= total - rows], np.int64)
    rng.shuffle(s)
    return s


def parity_cases():
    """codec x esz x ndims in full; per (codec, esz) the 14 ndims walk the chunk shapes and the data so that every value of
    every axis meets both codecs and both widths; each case runs all seven `rows` on both families"""
    cases = []
    for codec in ("delta", "xff"):
        for esz in (1, 2):
            for j, D in enumerate(NDIMS):
                shape = SHAPES[(j + esz + (codec == "xff")) % 3]
                data = DATA[(j + (1 if codec == "xff" else 0) + 2 * (esz - 1)) % 4]
                cases.append((codec, esz, D, shape, data))
    return cases


@pytest.mark.parametrize("codec,esz,D,shape,data", parity_cases())
def test_gather_rows_parity(sz, no_fast, codec, esz, D, shape, data):
    import torch
    rng = np.random.default_rng(zlib.crc32(f"{codec}{esz}{D}{shape}{data}".encode()))
    R = rows_per_chunk(shape, D)
    nchunks = 7 + D % 3
    total = nchunks * R - R // 3                           # every batch ends in a short last chunk
    x = gen_rows(data, rng, total, esz, D)
    cd, batch = compress(sz, codec, esz, D, R * D, x)
    for fam in (0, 1):
        no_fast(fam)
        for rk in ROWS:
            rows = rows_for(rk, R)
            starts = start_vector(rng, rows, R, total)
            assert starts.size >= 8
            rets = torch.full((starts.size,), -77, dtype=torch.int64, device="cuda")
            with gathers_on(fam, fast_shape_of(esz, D, R * D)):
                got = cd.gather_rows(batch, starts, rows, rets=rets)
            want, ok = gm.expected(x, starts, rows)
            assert ok.all()
            assert got.shape == (starts.size, rows, D) and got.dtype == cd.dtype
            assert np.array_equal(rets.cpu().numpy(), np.full(starts.size, rows)), (codec, esz, D, shape, data, fam, rk)
            g = got.cpu().numpy()
            bad = np.nonzero((g != want).reshape(starts.size, -1).any(axis=1))[0]
            assert bad.size == 0, (codec, esz, D, shape, data, fam, rk, rows, R, starts[bad].tolist())


# every lane mapping of decode_fast's gather mode (DP x CPL, EXACT or not), on chunks long enough for its read-ahead ring
FAST_MAPPINGS = [(2, 8), (2, 16), (2, 24), (2, 32), (2, 48), (2, 64), (2, 80), (2, 128), (2, 200), (2, 256),
                 (1, 16), (1, 32), (1, 48), (1, 64), (1, 80), (1, 128), (1, 208), (1, 256)]


@pytest.mark.parametrize("esz,D", FAST_MAPPINGS)
@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_gather_rows_fast_mappings(sz, no_fast, codec, esz, D):
    import torch
    rng = np.random.default_rng(D * 2 + esz)
    R = 16 * 11 + 5                                        # 181 rows: groups, runs and a verbatim tail
    nchunks = 9
    total = nchunks * R - 7
    x = gen_rows("walk", rng, total, esz, D)
    cd, batch = compress(sz, codec, esz, D, R * D, x)
    for fam in (0, 1):
        no_fast(fam)
        for rows in (1, 40, R + 9):
            starts = start_vector(rng, rows, R, total)
            with gathers_on(fam, True):                    # every mapping listed is decode_fast.h's
                got = cd.gather_rows(batch, starts, rows)
            want, ok = gm.expected(x, starts, rows)
            assert ok.all()
            bad = np.nonzero((got.cpu().numpy() != want).reshape(starts.size, -1).any(axis=1))[0]
            assert bad.size == 0, (codec, esz, D, fam, rows, starts[bad].tolist())


GUARD_SHAPES = [
    ("xff", 2, 8, 5120),          # decode_fast
    ("delta", 1, 80, 10240),      # decode_fast, 2 columns a lane
    ("delta", 1, 1, 1024),        # low-dim layout
    ("xff", 1, 3, 3000),          # low-dim layout, 3 columns
    ("delta", 2, 300, 9600),      # generic kernel
    ("xff", 2, 12, 1200),         # general layout, rows of 24 bytes: generic kernel
]
GUARD_FAST = {("xff", 2, 8, 5120), ("delta", 1, 80, 10240)}         # ... while d_out is 16-byte aligned


@pytest.mark.parametrize("codec,esz,D,chunk_len", GUARD_SHAPES)
@pytest.mark.parametrize("fam", [0, 1])
def test_gather_rows_output_guards(sz, no_fast, codec, esz, D, chunk_len, fam):
    """d_out carved out of a larger, sentinel-filled buffer, 16-byte aligned and element-aligned: every wanted element is
    written, the bytes in front and behind stay"""
    import torch
    from sprintz_amd import _lib
    no_fast(fam)
    rng = np.random.default_rng(D + fam)
    R = chunk_len // D
    nchunks = 6
    total = nchunks * R - 5
    x = gen_rows("walk", rng, total, esz, D)
    cd, batch = compress(sz, codec, esz, D, chunk_len, x)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for rows in (1, 9, R + 3):
        starts = np.array([R - 1, 0, total - rows, 2 * R, R + 1, 3], np.int64)
        d_starts = torch.from_numpy(starts).cuda()
        m = starts.size * rows * D * esz
        want, _ = gm.expected(x, starts, rows)
        for shift in (0, esz, 16 + esz):
            pad = 4096
            buf = torch.full((pad + shift + m + pad,), 0x5A, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            rets = torch.full((starts.size + 1,), -77, dtype=torch.int64, device="cuda")
            with gathers_on(fam, (codec, esz, D, chunk_len) in GUARD_FAST and shift % 16 == 0):
                _lib.check(_lib.gather_rows(_lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF, esz, batch.data.data_ptr(),
                                            batch.offsets.data_ptr(), nchunks, chunk_len, D, d_starts.data_ptr(), starts.size, rows,
                                            buf.data_ptr() + pad + shift, rets.data_ptr(), st))
            torch.cuda.synchronize()
            h = buf.cpu().numpy()
            assert np.all(h[:pad + shift] == 0x5A), (codec, D, rows, shift, "in front")
            assert np.all(h[pad + shift + m:] == 0x5A), (codec, D, rows, shift, "behind")
            assert np.array_equal(h[pad + shift:pad + shift + m].view(DTYPES[esz]).reshape(want.shape), want), (codec, D, rows, shift)
            r = rets.cpu().numpy()
            assert np.all(r[:-1] == rows) and r[-1] == -77


@pytest.mark.parametrize("codec,esz,D,chunk_len,quirk", [
    ("xff", 2, 8, 5120, 0),
    ("xff", 2, 8, 5120, 1),       # the reference decoder's run replay: what decompress writes with the option on
    ("xff", 2, 16, 2048, 1),
    ("xff", 2, 24, 2400, 1),      # decompress: the generic kernel
    ("delta", 1, 80, 10240, 0),
    ("delta", 1, 2, 1000, 0),
])
@pytest.mark.parametrize("fam", [0, 1])
def test_gather_rows_identity_with_decompress(sz, no_fast, codec, esz, D, chunk_len, quirk, fam):
    """starts = c R for every chunk, rows = R: bit for bit what decompress writes"""
    import torch
    from sprintz_amd import _lib
    rng = np.random.default_rng(chunk_len)
    R = chunk_len // D
    nchunks = 40
    x = gen_rows("walk", rng, nchunks * R, esz, D)          # data with runs
    if quirk:
        # an oscillation (the FIRE counters go negative), the decay FIRE predicts, 48 constant rows -- RUN blocks that start
        # with a non-zero prediction, where the reference decoder's replay differs from its encoder's -- then noise
        seq, v = [], 1000
        while len(seq) < nchunks * R:
            for i in range(8):
                v += 100 if i % 2 == 0 else -100
                seq.append(v)
            for dl in (6, -1, 0, 0, 0, 0, 0, 0):
                v += dl
                seq.append(v)
            seq += [v] * 48
            seq += list(rng.integers(0, 50, 32) + v)
        x = np.ascontiguousarray(np.repeat(np.mod(np.array(seq[:nchunks * R]), 65536).astype(np.uint16)[:, None], D, axis=1))
    cd, batch = compress(sz, codec, esz, D, chunk_len, x)
    no_fast(fam)
    _lib.check(_lib.set_option(_lib.OPT_REF_DECODER_QUIRK, quirk))
    try:
        dec = cd.decompress(batch)
        # (rows of 16 / 32 / 48 / 80 bytes are decode_fast.h's, whatever the quirk; the low-dim layout is not)
        with gathers_on(fam, D != 2):
            got = cd.gather_rows(batch, torch.arange(nchunks, dtype=torch.int64, device="cuda") * R, R)
        # and unaligned windows of it: rows the quirk has changed sit where decompress puts them
        starts = torch.tensor([5, R - 3, 7 * R + 11, 39 * R - 40], dtype=torch.int64, device="cuda")
        win = cd.gather_rows(batch, starts, 40)
    finally:
        _lib.set_option(_lib.OPT_REF_DECODER_QUIRK, 0)
    assert torch.equal(got.reshape(-1).view(torch.uint8), dec.view(torch.uint8))
    d2 = dec.view(torch.uint8).reshape(nchunks * R, D * esz)
    for i, s in enumerate(starts.tolist()):
        assert torch.equal(win[i].view(torch.uint8).reshape(40, D * esz), d2[s:s + 40]), (i, s)


FAIL_SHAPES = [
    ("xff", 2, 8, 5120, 0),       # decode_fast
    ("delta", 1, 80, 10240, 0),   # decode_fast, 2 columns a lane
    ("xff", 2, 8, 5120, 1),       # generic kernel
    ("delta", 1, 1, 1024, 0),     # low-dim layout
    ("delta", 2, 300, 9600, 0),
]


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", FAIL_SHAPES)
def test_gather_rows_missing_rows(sz, no_fast, codec, esz, D, chunk_len, fam):
    """a range past the end and one straddling the end of the short last chunk: negative entries, exact neighbours, nothing
    outside the failing ranges' own slots changes"""
    import torch
    no_fast(fam)
    rng = np.random.default_rng(11)
    R = chunk_len // D
    nchunks = 5
    total = nchunks * R - R // 2
    x = gen_rows("walk", rng, total, esz, D)
    cd, batch = compress(sz, codec, esz, D, chunk_len, x)
    rows = 24
    starts = np.array([7, total - 5, total - rows, nchunks * R + 9, R - 3, total, nchunks * R - 4, (1 << 62) + 5, total - rows - 1], np.int64)
    _, want_rets = gm.pieces(starts, rows, R, nchunks, gm.stream_rows(total * D, chunk_len, D))
    want, ok = gm.expected(x, starts, rows)
    assert np.array_equal(want_rets == rows, ok) and ok.sum() == 4
    sent = 0x5A if esz == 1 else 0x5A5A
    out = torch.full((starts.size, rows, D), sent, dtype=torch.int32, device="cuda").to(cd.dtype)
    rets = torch.full((starts.size,), -77, dtype=torch.int64, device="cuda")
    with gathers_on(fam, (codec, D) in (("xff", 8), ("delta", 80))):
        cd.gather_rows(batch, starts, rows, out=out, rets=rets, check=False)
    r = rets.cpu().numpy()
    assert np.array_equal(r, want_rets), (r, want_rets)
    g = out.cpu().numpy()
    assert np.array_equal(g[ok], want[ok])
    with pytest.raises(sz.SprintzError, match="range 1 "):
        cd.gather_rows(batch, starts, rows)
    # a failing range between two good ones in ONE buffer: the neighbours' rows around its slot are exact (checked above);
    # a range that fails without any of its rows existing writes nothing at all
    for i in (3, 5, 7):
        assert np.all(g[i] == sent), i


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", FAIL_SHAPES)
def test_gather_rows_damaged_chunks(sz, no_fast, codec, esz, D, chunk_len, fam):
    import torch
    no_fast(fam)
    rng = np.random.default_rng(5)
    R = chunk_len // D
    nchunks = 9
    total = nchunks * R
    x = gen_rows("uniform", rng, total, esz, D)            # incompressible: a row's bytes sit at row / R of the stream
    cd, batch = compress(sz, codec, esz, D, chunk_len, x)
    bad = 4
    off = int(batch.offsets[bad].item())
    size = int(batch.sizes[bad].item())
    rows = 10
    starts = np.array([bad * R - rows, bad * R - rows + 1, bad * R, bad * R + R // 2, (bad + 1) * R - 1, (bad + 1) * R, 0,
                       (bad - 1) * R - 1, bad * R + R - rows], np.int64)
    touches = (starts + rows > bad * R) & (starts < (bad + 1) * R)
    want, _ = gm.expected(x, starts, rows)

    # (a) a damaged header: every range touching the chunk fails, every other is exact
    hdr = batch.data[off + 6].clone()
    batch.data[off + 6] = hdr ^ 0x5                        # the header's ndims field
    rets = torch.full((starts.size,), -77, dtype=torch.int64, device="cuda")
    with gathers_on(fam, (codec, D) in (("xff", 8), ("delta", 80))):
        got = cd.gather_rows(batch, starts, rows, rets=rets, check=False)
    r = rets.cpu().numpy()
    assert np.all(r[touches] < 0) and np.all(r[~touches] == rows), r
    assert np.array_equal(got.cpu().numpy()[~touches], want[~touches])
    first_bad = int(np.nonzero(touches)[0][0])
    with pytest.raises(sz.SprintzError, match=f"range {first_bad} "):
        cd.gather_rows(batch, starts, rows)
    batch.data[off + 6] = hdr
    assert np.array_equal(cd.gather_rows(batch, starts, rows).cpu().numpy(), want)     # repaired: no error

    # (b) damage behind row k only: ranges that end before k in that chunk are exact and delivered
    k = R // 2
    lo_b = off + size * 3 // 4                             # bytes of rows well past k (the stream is ~ 1 : 1 with the rows)
    saved = batch.data[lo_b:off + size].clone()
    batch.data[lo_b:off + size] = saved ^ 0xFF
    early = np.array([bad * R, bad * R + k - rows, bad * R - 3, bad * R + 1, (bad + 1) * R + 2, bad * R + k // 2], np.int64)
    rets = torch.full((early.size,), -77, dtype=torch.int64, device="cuda")
    got = cd.gather_rows(batch, early, rows, rets=rets, check=False)
    w2, _ = gm.expected(x, early, rows)
    assert np.all(rets.cpu().numpy() == rows), rets
    assert np.array_equal(got.cpu().numpy(), w2)
    batch.data[lo_b:off + size] = saved


@pytest.mark.parametrize("fam", [0, 1])
def test_read_rows_over_3000_chunks(sz, no_fast, fam):
    import torch
    no_fast(fam)
    rng = np.random.default_rng(8)
    D, R, nchunks = 8, 640, 3000
    total = nchunks * R - 77
    x = gen_rows("walk", rng, total, 2, D)
    cd, batch = compress(sz, "xff", 2, D, R * D, x)
    with gathers_on(fam, True):                               # uint16 x 8: rows of 16 bytes
        got = cd.read_rows(batch, 1, total - 1)
    assert got.shape == (total - 2, D)
    assert np.array_equal(got.cpu().numpy(), x[1:total - 1])
    assert np.array_equal(cd.read_rows(batch, 5 * R - 1, 5 * R + 1).cpu().numpy(), x[5 * R - 1:5 * R + 1])
    with pytest.raises(sz.SprintzError):
        cd.read_rows(batch, total - 3, total + 1)


@pytest.mark.parametrize("name,nranges,rows", [("cfg2", 65536, 256), ("cfg3_10k", 16384, 256), ("cfg1", 16384, 256)])
def test_gather_rows_bench_sizes(sz, name, nranges, rows):
    """the bench's own inputs at full size, random starts, every range compared with the input's rows"""
    import torch
    from rowdata import bench_input
    (codec, esz, D, chunk_len, nchunks), x = bench_input(name, "cuda:0")
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device="cuda:0")
    batch = cd.compress(x)
    total = nchunks * (chunk_len // D)
    g = torch.Generator(device="cuda")
    g.manual_seed(17)
    starts = torch.randint(0, total - rows + 1, (nranges,), generator=g, device="cuda", dtype=torch.int64)
    got = cd.gather_rows(batch, starts, rows)
    xi = x.view(torch.int8 if esz == 1 else torch.int16).view(total, D)
    step = 4096
    for i in range(0, nranges, step):                      # torch indexes the signed view: same bits
        idx = starts[i:i + step, None] + torch.arange(rows, device="cuda")[None, :]
        assert torch.equal(got[i:i + step].view(xi.dtype), xi[idx]), (name, i)


def test_gather_rows_beyond_4_GiB(sz):
    """520 000 mostly incompressible chunks: the container passes 2^32 bytes, so the call runs on the kernel with plain
    64-bit addresses -- ranges in the first and the last chunks; then an output above 4 GiB, first and last ranges checked"""
    import torch
    n, chunk_len, D = 520000, 5120, 8
    R = chunk_len // D
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    x = torch.randint(0, 65536, (n * chunk_len,), generator=g, device="cuda", dtype=torch.int32).to(torch.uint16)
    xv = x.view(torch.int16).view(n, chunk_len)
    xv[::4] = xv[::4] & 0x00ff
    cd = sz.ChunkedCodec("xff", 2, D, chunk_len)
    batch = cd.compress(x)
    assert batch.total_bytes() > (1 << 32) + (1 << 28)
    rows2d = x.view(torch.int16).view(n * R, D)
    total = n * R
    starts = torch.tensor([0, 3, R - 1, 2 * R + 5, total - 700, total - 2 * R - 1, total - R - 700, total - 705, (n // 2) * R + 17],
                          dtype=torch.int64, device="cuda")
    got = cd.gather_rows(batch, starts, 700)
    for i, s in enumerate(starts.tolist()):
        assert torch.equal(got[i].view(torch.int16), rows2d[s:s + 700]), (i, s)
    del got
    # the output above 4 GiB on a container below it: the headline shape's first 140 000 chunks would do, but the data is here
    # already -- 1 100 ranges of 245 760 rows (384 chunks each): 4.33 GB delivered
    rows = 384 * R
    nr = 1100
    starts = (torch.arange(nr, dtype=torch.int64, device="cuda") * 397 * R + 5) % (total - rows)
    out = cd.gather_rows(batch, starts, rows)
    assert out.numel() * 2 > (1 << 32)
    for i in (0, 1, nr // 2, nr - 2, nr - 1):
        s = int(starts[i].item())
        assert torch.equal(out[i].view(torch.int16), rows2d[s:s + rows]), (i, s)
