"""GPU tests (-m gpu) of the planner's eligibility predicates (csrc/plan.h: plan_decode, plan_encode, plan_gather, plan_dense) as the
launchers of csrc/api.hip run them: for every edge, the last shape that takes a kernel and the first that does not -- where a
predicate that is off by one sends a shape to a kernel that cannot handle it, or keeps a kernel from every shape it was written for.  Each case is one small valid batch of a walk with flat
spans: compress -> the oracle's bytes for every chunk -> decompress -> the input, every return value -- and, from the dispatch counters
(tests/dispatch.py), the kernel family on both sides of the edge.  The expectations are literals, read off the "Shapes" paragraphs of the
kernels' headers and the options' text in sprintz_mi355x.h; the comments say which term of the predicate the pair straddles.  The table
lives in tests/dispatch_cases.py: the CPU tier replays it through the planner alone (tests/test_plan_cpu.py).

Then containers larger than 4 GiB on decode_row.h (a batch that is a sub-range of one, addressed from the container's base), and a
batch whose OUTPUT passes 4 GB, which that kernel leaves to the older ones."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from dispatch import ran
from dispatch_cases import CASES, ENC, GATHER_EDGES
from harness import DTYPES, gen_walk
from fixtures import sz  # noqa: F401  (fixtures)
from streams import check_streams

pytestmark = pytest.mark.gpu


@contextmanager
def options(lat=2048, blk_chunks=2049, mask=9, pair=1):
    """the four knobs the row-major dispatch reads, at the library's defaults unless given (pair: the test session's, tests/conftest.py)"""
    from sprintz_amd import _lib
    knobs = [(_lib.OPT_LAT_CHUNKS, lat, "SPRINTZ_MI355X_LAT_CHUNKS", 2048), (_lib.OPT_BLK_CHUNKS, blk_chunks, "SPRINTZ_MI355X_BLK_CHUNKS", 2049),
             (_lib.OPT_BLK_KERNELS, mask, "SPRINTZ_MI355X_BLK_KERNELS", 9), (_lib.OPT_ENC_PAIR, pair, "SPRINTZ_MI355X_ENC_PAIR", 1024)]
    for opt, v, _, _ in knobs:
        _lib.check(_lib.set_option(opt, v))
    try:
        yield
    finally:
        for opt, _, env, default in knobs:
            _lib.set_option(opt, int(os.environ.get(env, default)))


def make_batch(sz, codec, esz, D, chunk_len, nchunks, align=16, seed=0):
    import torch
    rng = np.random.default_rng(1000 * D + chunk_len + esz + seed)
    data = gen_walk(rng, nchunks * chunk_len, D, esz, 3, flat_every=2)
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device="cuda:0", align=align)
    t = torch.from_numpy(data.view(np.int8 if esz == 1 else np.int16)).cuda().view(cd.dtype)
    return data, cd, t


def roundtrip(sz, oracle, codec, esz, D, chunk_len, nchunks, enc=None, dec=None, align=16, src_shift=0, out_shift=0, comp_shift=0, tag=""):
    """enc: {family: launches} of the compress call, nothing else may move; dec: the one family of the decompress call"""
    import torch
    from sprintz_amd import _lib
    data, cd, t = make_batch(sz, codec, esz, D, chunk_len, nchunks, align)
    n = data.size
    if src_shift or align != 16:                        # a source that starts src_shift bytes behind a 16-byte boundary: the slot path (compress() copies its input)
        buf = torch.zeros(16 + n * esz + _lib.READ_SLACK, dtype=torch.uint8, device="cuda:0")
        buf[src_shift:src_shift + n * esz] = t.view(torch.uint8)
        src = buf[src_shift:]
        assert src.data_ptr() % 16 == src_shift
        with ran(only=list(enc), what=tag, **enc) if enc else ran():
            ws = cd.compress_to_slots(src, n)
            dense, offsets = cd.compact(ws, nchunks)
        sizes_t = ws["sizes"]
    else:
        with ran(only=list(enc), what=tag, **enc) if enc else ran():
            batch = cd.compress(t)
        dense, offsets, sizes_t = batch.data, batch.offsets, batch.sizes
    total = int(offsets[-1].item())
    check_streams(oracle, codec, data, chunk_len, D, dense[:total].cpu().numpy(), offsets.cpu().numpy(), sizes_t.cpu().numpy(), tag)
    cbuf = torch.zeros(comp_shift + total + _lib.READ_SLACK, dtype=torch.uint8, device="cuda:0")      # the container, comp_shift bytes behind an aligned address
    cbuf[comp_shift:comp_shift + total] = dense[:total]
    obuf = torch.full((n + 16,), 0x5A, dtype=torch.int8 if esz == 1 else torch.int16, device="cuda:0").view(cd.dtype)
    out = obuf[out_shift:out_shift + n]                 # the output, out_shift ELEMENTS behind an aligned address
    assert cbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
    rets = torch.full((nchunks,), -77, dtype=torch.int64, device="cuda:0")
    with ran(only=[dec], what=tag, **{dec: 1}) if dec else ran():
        cd.decompress_into(cbuf[comp_shift:], offsets, nchunks, out, rets)
    assert (rets.cpu().numpy() == chunk_len).all(), (tag, rets[:8])
    o = obuf.cpu().numpy().view(DTYPES[esz])
    assert np.array_equal(o[out_shift:out_shift + n], data), tag
    assert (o[:out_shift] == 0x5A).all() and (o[out_shift + n:] == 0x5A).all(), (tag, "wrote outside the output")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_both_sides_of_every_edge(sz, oracle, case):
    tag, opts, codec, esz, D, chunk_len, nchunks, enc, dec, kw = case
    with options(**opts):
        roundtrip(sz, oracle, codec, esz, D, chunk_len, nchunks, enc=enc, dec=dec, tag=tag, **kw)


@pytest.mark.parametrize("write_size,family", [(True, "enc_blk"), (False, "enc_pair")])
def test_encode_blk_writes_the_stream_header_itself(sz, oracle, write_size, family):
    """write_size = 0 (a single call's headerless stream): encode_blk.h always writes the 8-byte header, so the call stays on the older
    encoder; with the header it is encode_blk.h's from one chunk on"""
    rng = np.random.default_rng(16)
    D, n = 16, 2048
    data = gen_walk(rng, n, D, 1, 3, flat_every=2)
    want, wret = oracle.compress("delta", data, D, write_size=write_size)
    dest = np.full(n * 2 + 512, 0xAB, np.uint8)
    with options(**ENC):
        with ran(only=[family], **{family: 1}):
            ret = sz.sprintz_compress_delta_8b(data, n, dest, D, write_size)
    assert ret == wret and np.array_equal(dest[:want.size], want) and (dest[want.size + 64:] == 0xAB).all()
    full, _ = oracle.compress("delta", data, D)
    out = np.zeros(n + 64, np.uint8)
    if write_size:
        assert sz.sprintz_decompress_delta_8b(dest, out) == n
    else:
        ngroups, remaining = int(np.frombuffer(full[:4].tobytes(), np.uint32)[0]), int(np.frombuffer(full[4:6].tobytes(), np.uint16)[0])
        assert sz.decompress_noheader("delta", 1, want, out, D, ngroups, remaining) == n
    assert np.array_equal(out[:n], data)


@pytest.mark.parametrize("esz,D,out_shift,family", GATHER_EDGES)
def test_gather_rows_edges(sz, esz, D, out_shift, family):
    """decode_fast.h's gather mode stores 16-byte pieces of rows: rows of whole pieces into a 16-byte aligned output; everything else is
    the generic kernel's"""
    import torch
    R, nchunks, rows = 64, 9, 70
    data, cd, t = make_batch(sz, "xff", esz, D, R * D, nchunks)
    batch = cd.compress(t)
    starts = np.array([0, R - 1, 3 * R + 5, nchunks * R - rows, 2 * R, 17], np.int64)
    m = starts.size * rows * D
    obuf = torch.full((m + 32,), 0x5A, dtype=torch.int8 if esz == 1 else torch.int16, device="cuda:0").view(cd.dtype)
    assert obuf.data_ptr() % 16 == 0
    rets = torch.full((starts.size,), -77, dtype=torch.int64, device="cuda:0")
    with ran(only=[family], **{family: 1}):
        got = cd.gather_rows(batch, starts, rows, out=obuf[out_shift:out_shift + m], rets=rets)
    assert (rets.cpu().numpy() == rows).all()
    x = data.reshape(nchunks * R, D)
    want = np.stack([x[s:s + rows] for s in starts])
    assert np.array_equal(got.cpu().numpy().view(DTYPES[esz]), want)
    o = obuf.cpu().numpy().view(DTYPES[esz])
    assert (o[:out_shift] == 0x5A).all() and (o[out_shift + m:] == 0x5A).all()


# ------------------------------------------------------------------ containers past 4 GiB

@pytest.fixture(scope="module")
def big_buffer():
    """2^32 + 2^26 zero bytes on the device, shared by the cases below (each writes its container into it and clears it again)"""
    import torch
    big = torch.zeros((1 << 32) + (1 << 26), dtype=torch.uint8, device="cuda:0")
    yield big
    del big
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mask", [9, 25])
@pytest.mark.parametrize("esz,D,chunk_len,nchunks", [(1, 32, 1024, 24), (1, 80, 10240, 12)])
@pytest.mark.parametrize("where", ["past", "straddles", "control"])
def test_decode_row_reads_a_batch_anywhere_in_a_large_container(sz, oracle, big_buffer, where, esz, D, chunk_len, nchunks, mask):
    """A valid batch that is a sub-range of a container larger than 4 GiB, addressed from the container's base: d_offsets are the caller's, the
    header sets no limit on them and allows padding between streams.  decode_row.h once kept 32-bit container offsets and reported every
    stream with offset + length >= 0xfffffff0 as SPRINTZ_E_CORRUPT; its launch guard bounded what this library's compaction writes, not
    what a caller passes.  B: every stream past 2^32; the batch straddling 2^32; and 4 096 as the control.  A second control passes
    the view big[B:] with the batch's own offsets."""
    import torch
    data, cd, t = make_batch(sz, "delta", esz, D, chunk_len, nchunks)
    with options(lat=0, blk_chunks=1, mask=mask):
        batch = cd.compress(t)
        total = int(batch.offsets[-1].item())
        check_streams(oracle, "delta", data, chunk_len, D, batch.data[:total].cpu().numpy(), batch.offsets.cpu().numpy(), batch.sizes.cpu().numpy(), where)
        B = {"past": (1 << 32) + 4096, "straddles": ((1 << 32) - total // 2) & ~3, "control": 4096}[where]
        assert B % 4 == 0 and B + total + 16 <= big_buffer.numel()
        if where == "straddles":
            offs = batch.offsets.cpu().numpy()
            assert B + offs[0] < (1 << 32) - 16 < (1 << 32) < B + offs[-1]
        big_buffer[B:B + total] = batch.data[:total]
        try:
            for comp, offsets in ((big_buffer, batch.offsets + B), (big_buffer[B:], batch.offsets)):
                out = torch.full((nchunks * chunk_len,), 0x5A, dtype=torch.uint8, device="cuda:0")
                rets = torch.full((nchunks,), -77, dtype=torch.int64, device="cuda:0")
                with ran(dec_row=1, only=["dec_row"]):
                    cd.decompress_into(comp, offsets, nchunks, out, rets)
                r = rets.cpu().numpy()
                assert (r == chunk_len).all(), (where, B, r)
                assert np.array_equal(out.cpu().numpy(), data), (where, B)
        finally:
            big_buffer[B:B + total] = 0


def test_an_output_of_4_GB_stays_on_the_older_kernel(sz):
    """decode_row.h addresses its OUTPUT with 32-bit offsets: a batch that decodes to 0xf0000000 bytes or more is the lane-per-column
    kernel's, and is counted there; one chunk less is decode_row.h's"""
    import torch
    D, chunk_len = 32, 32768
    nchunks = 0xf0000000 // chunk_len                                       # 122 880 chunks: exactly 0xf0000000 bytes
    rng = np.random.default_rng(4)
    tile = torch.from_numpy(gen_walk(rng, 64 * chunk_len, D, 1, 3, flat_every=2)).cuda()
    x = tile.repeat(nchunks // 64)
    assert x.numel() == 0xf0000000
    cd = sz.ChunkedCodec("delta", 1, D, chunk_len, device="cuda:0")
    with options(lat=0, blk_chunks=1, mask=9):
        batch = cd.compress(x)
        out = torch.empty(nchunks * chunk_len, dtype=torch.uint8, device="cuda:0")
        rets = torch.empty(nchunks, dtype=torch.int64, device="cuda:0")
        with ran(dec_fast=1, only=["dec_fast"]):
            cd.decompress_into(batch.data, batch.offsets, nchunks, out, rets)
        assert bool((rets == chunk_len).all()) and torch.equal(out, x)
        out.zero_()
        rets.zero_()
        with ran(dec_row=1, only=["dec_row"]):
            cd.decompress_into(batch.data, batch.offsets, nchunks - 1, out, rets)
        n1 = (nchunks - 1) * chunk_len
        assert bool((rets[:-1] == chunk_len).all()) and torch.equal(out[:n1], x[:n1]) and not bool(out[n1:].any())
