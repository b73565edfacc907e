"""GPU tests (-m gpu): the FIRE forecaster's counters driven through their extremes on EVERY kernel that carries them.

The 8-bit codec's counter is an int16 that wraps (reference util.h:39-47; _mm256_add_epi16 in sprintz_xff_rle.cpp:1067,
sprintz_xff_lowdim.cpp:965, predict.cpp:202); every FIRE kernel restates that wrap by hand (wrap_counter<8>, csrc/sprintz_device.h, and
xff_kernel's own copy in csrc/transforms.hip).  The 16-bit low-dim coefficient (ctr >> 1, untruncated) passes 2^23, where it no longer
fits the 24-bit multiply fire_predict uses everywhere else.  The inputs are tests/fire_drive.py's: every 8-bit column wraps, both ways,
with run spans at frozen extreme coefficients before and behind the wrap (tests/test_fire_extremes_cpu.py asserts that they do).

Every case: compress -> the oracle's bytes for every chunk -> decompress -> the input and every return value, and the kernel family on
both sides from the dispatch counters (tests/dispatch.py); the families are read off csrc/plan.h's plan_decode / plan_encode.  A
batch holds 5 to 7 chunks with seeds and direction patterns of their own, so that the lanes of a wave sit at different counter states;
its first chunk is the golden fixture's case (tests/golden/golden_firewrap_v1, minted from the compiled reference by
oracle/gen_golden_firewrap.py) where there is one, and is compared with the reference's bytes too.  Nothing here needs the reference or anything built from its sources."""
import json
import os
import zlib

import numpy as np
import pytest

import fire_drive as fd
import window_model as wm
from dispatch import ran
from harness import DTYPES
from fixtures import sz  # noqa: F401  (fixtures)
from streams import DEF, DENSE, GENERIC, OLD, check_streams, fire_batch_of as batch_of, fire_oracle_batch as oracle_batch, options, to_device

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_firewrap_v1")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN + ".json") as f:
        manifest = json.load(f)["cases"]
    arrays = np.load(GOLDEN + ".npz")
    return {(m["what"], m["w"], m["ndims"]): (m, arrays[m["name"]]) for m in manifest}


def check_golden(golden, what, w, D, x, got):
    """the batch's first chunk is the fixture's input (its CRC32 says so): the device wrote the compiled reference's bytes"""
    if (what, w, D) not in golden:
        return False
    m, want = golden[(what, w, D)]
    assert x.size == m["n"] and zlib.crc32(x.tobytes()) == m["input_crc32"], (m, "not the fixture's input")
    assert got.size == want.size and np.array_equal(got, want), (m, "differs from the compiled reference's bytes")
    return True


def roundtrip(sz, oracle, golden, w, D, nchunks, enc, dec, tag, nblocks=None, runs=None):
    """enc / dec: the one family of the compress / decompress call; of the others only the container's may move"""
    import torch
    esz = w // 8
    data, chunk_len = batch_of(w, D, nchunks, nblocks, runs)
    n = data.size
    cd = sz.ChunkedCodec("xff", esz, D, chunk_len, device="cuda:0")
    t = to_device(cd, data)
    with ran(only=[enc, *DENSE], what=tag, **{enc: 1}):
        batch = cd.compress(t)
    total = int(batch.offsets[-1].item())
    comp, offs, sizes = batch.data[:total].cpu().numpy(), batch.offsets.cpu().numpy(), batch.sizes.cpu().numpy()
    check_streams(oracle, "xff", data, chunk_len, D, comp, offs, sizes, tag)
    if nblocks is None:
        check_golden(golden, "codec", w, D, data[:chunk_len], comp[offs[0]:offs[0] + sizes[0]])
    obuf = torch.full((n + 16,), 0x5A, dtype=torch.int8 if esz == 1 else torch.int16, device="cuda:0").view(cd.dtype)
    rets = torch.full((nchunks,), -77, dtype=torch.int64, device="cuda:0")
    with ran(only=[dec], what=tag, **{dec: 1}):
        cd.decompress_into(batch.data, batch.offsets, nchunks, obuf[:n], rets)
    assert (rets.cpu().numpy() == chunk_len).all(), (tag, rets)
    o = obuf.cpu().numpy().view(DTYPES[esz])
    bad = np.flatnonzero(o[:n] != data)
    assert bad.size == 0, (tag, "first wrong sample: chunk", int(bad[0]) // chunk_len, "row", (int(bad[0]) % chunk_len) // D, "column", int(bad[0]) % D)
    assert (o[n:] == 0x5A).all(), (tag, "wrote outside the output")
    return batch


# 8-bit xff, chunks of 9 280 rows (1 160 blocks): id, options, ndims, chunks, encoder, decoder
CASES8 = [
    # ---- low-dim layout
    ("lat D=1: 9 280-byte chunks", DEF, 1, 7, "enc_lat", "dec_lat"),
    ("lat D=2: 18 560-byte chunks inside the 150 KB carve (at most 64 chunks)", DEF, 2, 6, "enc_lat", "dec_lat"),
    ("uni D=1", OLD, 1, 7, "enc_uni", "dec_uni"),
    ("uni D=2", OLD, 2, 6, "enc_uni", "dec_uni"),
    ("uni D=3", OLD, 3, 5, "enc_uni", "dec_uni"),
    ("uni D=4", OLD, 4, 7, "enc_uni", "dec_uni"),
    # ---- general layout, a lane per column or column pair
    ("pair D=8: DP 8, exact", OLD, 8, 7, "enc_pair", "dec_fast"),
    ("fast D=8: one column a lane (ENC_PAIR 0)", dict(OLD, pair=0), 8, 7, "enc_fast", "dec_fast"),
    ("pair D=6: lane group not full", OLD, 6, 5, "enc_pair", "dec_fast"),
    ("fast D=6 (ENC_PAIR 0)", dict(OLD, pair=0), 6, 5, "enc_fast", "dec_fast"),
    ("pair D=32", OLD, 32, 6, "enc_pair", "dec_fast"),
    ("pair D=64", OLD, 64, 5, "enc_pair", "dec_fast"),
    ("split D=80: pair + single column a lane, decode 32 x 3", OLD, 80, 5, "enc_split", "dec_fast"),
    ("wide D=80 on 64 lanes x 2 (SPLIT_LANES 0)", dict(OLD, split=0), 80, 5, "enc_wide", "dec_fast"),
    ("wide D=96: two columns a lane", OLD, 96, 5, "enc_wide", "dec_fast"),
    # (decode_fast.h addresses a wavefront's span of the output with 32-bit offsets: chunk bytes x 4 096 = 1 187 840 x 4 096 >= 0xf0000000)
    ("wide D=128, exact; decode leaves decode_fast.h", OLD, 128, 5, "enc_wide", "dec_generic"),
    # (blocks of 40 bytes are no whole 16-byte pieces: blk_bytes % 16 on both sides)
    ("generic D=5: 40-byte blocks", OLD, 5, 6, "enc_generic", "dec_generic"),
    ("generic D=1 (NO_FAST)", GENERIC, 1, 7, "enc_generic", "dec_generic"),
    ("generic D=8 (NO_FAST)", GENERIC, 8, 7, "enc_generic", "dec_generic"),
    # ---- more than 512 columns: a workgroup per chunk (any_ndims.hip); from 2 048 on the counters live in scratch memory
    ("any D=600", OLD, 600, 2, "enc_any", "dec_any"),
    ("big D=2048", OLD, 2048, 1, "enc_big", "dec_big"),
]


@pytest.mark.parametrize("case", CASES8, ids=[c[0] for c in CASES8])
def test_8_bit_counters_wrap_on_every_kernel(sz, oracle, golden, case):
    tag, opts, D, nchunks, enc, dec = case
    with options(**opts):
        roundtrip(sz, oracle, golden, 8, D, nchunks, enc, dec, tag)


CASES16 = [
    ("uni u16 D=1", OLD, 1, 5, "enc_uni", "dec_uni"),
    ("uni u16 D=2", OLD, 2, 5, "enc_uni", "dec_uni"),
    ("generic u16 D=1 (NO_FAST)", GENERIC, 1, 5, "enc_generic", "dec_generic"),
    ("generic u16 D=2 (NO_FAST)", GENERIC, 2, 5, "enc_generic", "dec_generic"),
]


@pytest.mark.parametrize("case", CASES16, ids=[c[0] for c in CASES16])
def test_16_bit_low_dim_coefficient_past_2_to_23(sz, oracle, golden, case):
    """35 200 rows: counters of +-36 M, coefficients of +-18 M -- the W == 16 && LOWDIM branch of fire_predict, a full 32-bit product"""
    tag, opts, D, nchunks, enc, dec = case
    with options(**opts):
        roundtrip(sz, oracle, golden, 16, D, nchunks, enc, dec, tag)


@pytest.mark.parametrize("w,D,nblocks,runs", [(8, 8, 256, ((200, 204),)), (16, 1, 1024, ((900, 920),))])
def test_workgroup_per_chunk_kernels_as_far_as_their_chunks_reach(sz, oracle, golden, w, D, nblocks, runs):
    """encode_lat.h / decode_lat.h keep a whole chunk in LDS, with 4 bytes an element of working set: a GENERAL-layout chunk long enough to
    wrap (5 columns x 8 200 rows x 4 bytes) exceeds the 150 KB carve, so only the low-dim cases above wrap there.  These give the general
    layout what it takes: 8 columns in chunks of 16 384 elements (256 blocks: counters of +-8 000, 16 times what the walks reach), and
    16-bit univariate chunks of 8 192 elements (1 024 blocks: coefficients of +-4 M)"""
    data, chunk_len = batch_of(w, D, 6, nblocks, runs)
    ctr = np.concatenate([fd.chunk(w, D, k, (2, 3, 0, 1, 4, 5)[k], runs, nblocks)[1] for k in range(6)], axis=1)
    assert chunk_len == 8 * nblocks * D and np.abs(ctr).max() >= (8000 if w == 8 else 8_000_000)
    with options(**DEF):
        roundtrip(sz, oracle, golden, w, D, 6, "enc_lat", "dec_lat", f"lat w={w} D={D}", nblocks, runs)


@pytest.mark.parametrize("D", [1, 8])
def test_single_calls(sz, oracle, golden, D):
    """sprintz_compress_xff_8b / sprintz_decompress_xff_8b on the fixture's inputs: the reference's bytes and return value, nothing written behind them"""
    x = fd.codec_input(8, D)
    n = x.size
    want, wret = oracle.compress("xff", x, D)
    dest = np.full(n * 2 + 512, 0xAB, np.uint8)
    ret = sz.sprintz_compress_xff_8b(x, n, dest, D, True)
    assert ret == wret == golden[("codec", 8, D)][0]["ret"], (ret, wret, sz.last_error())
    assert np.array_equal(dest[:want.size], want) and (dest[want.size:] == 0xAB).all()
    assert check_golden(golden, "codec", 8, D, x, dest[:want.size])
    out = np.full(n + 64, 0xCD, np.uint8)
    assert sz.sprintz_decompress_xff_8b(golden[("codec", 8, D)][1], out) == n
    assert np.array_equal(out[:n], x) and (out[n:] == 0xCD).all()


@pytest.mark.parametrize("D,family", [(16, "gather_fast"), (1, "gather_generic")])
def test_gather_rows_behind_the_wrap(sz, oracle, D, family):
    """row ranges that lie wholly behind every column's wrap (rows from 8 500 on; the last column wraps at block 1 088, row 8 704, and the
    decoder has to carry the counters there from the chunk's start), two of them straddling the edges of the late run span (blocks 1 100 ..
    1 119: rows 8 800 .. 8 959), one ending with the chunk.  The container holds the oracle's streams"""
    import torch
    nchunks, rows, R = 5, 120, 8 * fd.NB8
    data, chunk_len = batch_of(8, D, nchunks)
    assert chunk_len == R * D and fd.RUNS8[-1] == (1100, 1120)
    cd = sz.ChunkedCodec("xff", 1, D, chunk_len, device="cuda:0")
    with options(**OLD):
        batch = oracle_batch(sz, oracle, D, data, chunk_len)
        starts = np.array([c * R + s for c, s in ((0, 8500), (1, 8760), (2, 8900), (3, R - rows), (4, 8704), (0, 8790))], np.int64)
        rets = torch.full((starts.size,), -77, dtype=torch.int64, device="cuda:0")
        with ran(only=[family], **{family: 1}):
            got = cd.gather_rows(batch, starts, rows, rets=rets)
    assert (rets.cpu().numpy() == rows).all()
    x = data.reshape(nchunks * R, D)
    assert np.array_equal(got.cpu().numpy(), np.stack([x[s:s + rows] for s in starts]))


@pytest.mark.parametrize("D,opts,family", [(8, OLD, "dec_fast"), (1, OLD, "dec_uni"), (8, GENERIC, "dec_generic")])
def test_windowed_query(sz, oracle, D, opts, family):
    """per-window min / max / sum fused into the decoders' query forms: 145 windows of 64 rows a chunk of the oracle's streams, against the model
    applied to the input"""
    nchunks = 5
    data, chunk_len = batch_of(8, D, nchunks)
    cd = sz.ChunkedCodec("xff", 1, D, chunk_len, device="cuda:0")
    with options(**opts):
        batch = oracle_batch(sz, oracle, D, data, chunk_len)
        with ran(only=[family], **{family: 1}):
            got = cd.query_windows(batch, 64, per_chunk=True)
    mn, mx, sm = wm.chunk_windows(data, chunk_len, D, 64)
    assert np.array_equal(got["min"].cpu().numpy(), mn) and np.array_equal(got["max"].cpu().numpy(), mx)
    assert np.array_equal(got["sum"].cpu().numpy().view(np.uint64), sm)


@pytest.mark.parametrize("D", [1, 8, 33])
def test_transform(sz, oracle, golden, D):
    """transform_device("xff"): xff_kernel's own copy of the wrap (csrc/transforms.hip), on inputs steered against ITS forecast (the previous
    delta unsigned in even columns): the oracle's errors, the compiled reference's container where the fixture has one, and the input back"""
    import torch
    x = fd.transform_input(D)
    assert x.size == 8 * fd.NB8 * D + 5
    want, _ = oracle.transform_encode(2, x, D)
    xd = torch.from_numpy(x.copy()).cuda()
    y = sz.transform_device("xff", xd, D)
    got = y.cpu().numpy()
    assert np.array_equal(got, want[6:])
    if ("transform", 8, D) in golden:
        assert check_golden(golden, "transform", 8, D, x, np.concatenate([want[:6], got]))
    else:
        assert D == 33
    back = sz.transform_device("xff", y, D, inverse=True)
    assert torch.equal(back, xd)
