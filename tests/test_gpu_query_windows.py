"""GPU tests (-m gpu) of the windowed query (sprintz_mi355x_query_windows, ChunkedCodec.query_windows): per-window
min / max / sum fused into the three decoder families (decode_fast.h, decode_uni.h, decode_kernel.h).  The expected value
is always tests/window_model.py applied to the ORIGINAL input -- decode is lossless and pinned elsewhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import window_model as wm
from fixtures import no_fast, sz  # noqa: F401  (fixtures)
from rowdata import chunk_len_for, gen_data, make_batch, parity_cases

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

pytestmark = pytest.mark.gpu

WKINDS = ["8", "24", "64", "R", ">R"]


def window_for(kind, chunk_len, D):
    R = -(-chunk_len // D)
    r8 = -(-R // 8) * 8
    return {"8": 8, "24": 24, "64": 64, "R": r8, ">R": r8 + 8}[kind]


def assert_windows(got, want, msg):
    mn, mx, sm = want
    assert np.array_equal(got["min"].cpu().numpy().astype(np.int64), mn.astype(np.int64)), ("min",) + msg
    assert np.array_equal(got["max"].cpu().numpy().astype(np.int64), mx.astype(np.int64)), ("max",) + msg
    assert np.array_equal(got["sum"].cpu().numpy().view(np.uint64), sm), ("sum",) + msg


@pytest.mark.parametrize("codec,esz,D,shape,data,general", parity_cases())
def test_query_windows_parity(sz, oracle, no_fast, codec, esz, D, shape, data, general):
    import zlib
    rng = np.random.default_rng(zlib.crc32(f"{codec}{esz}{D}{shape}{data}{general}".encode()))
    chunk_len = chunk_len_for(shape, D)
    nchunks = 5 + D % 4
    n = nchunks * chunk_len - chunk_len // 3 - 1          # every batch ends in a short last chunk
    x = gen_data(data, rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, general)
    for fam in (0, 1):
        no_fast(fam)
        for wk in WKINDS:
            W = window_for(wk, chunk_len, D)
            got = cd.query_windows(batch, W, general_layout=general, per_chunk=True)
            assert_windows(got, wm.chunk_windows(x, chunk_len, D, W), (codec, esz, D, shape, data, general, fam, wk, W))


@pytest.mark.parametrize("codec,esz,D,chunk_len", [
    ("xff", 2, 8, 5120),          # decode_fast
    ("delta", 1, 1, 1024),        # decode_uni
    ("xff", 1, 3, 3001),          # decode_uni, 3 columns, ragged
    ("delta", 2, 300, 9677),      # decode_kernel
])
def test_query_windows_output_guards(sz, oracle, codec, esz, D, chunk_len):
    """sentinel-filled, padded outputs: nothing lands past nchunks*nwin*ndims, every entry is written, and an op that is
    not selected may have a NULL output"""
    import torch
    from sprintz_amd import _lib
    rng = np.random.default_rng(D)
    nchunks = 7
    n = nchunks * chunk_len - chunk_len // 2
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    dt = torch.uint8 if esz == 1 else torch.uint16
    sent = 0x5A if esz == 1 else 0x5A5A
    for W in (8, 64):
        want = wm.chunk_windows(x, chunk_len, D, W)
        m = want[0].size
        pad = 4096
        for ops in (7, 1, 2, 4, 5, 6, 3):
            mn = torch.full((m + pad,), sent, dtype=torch.int32, device="cuda").to(dt)
            mx = torch.full((m + pad,), sent, dtype=torch.int32, device="cuda").to(dt)
            sm = torch.full((m + pad,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
            rets = torch.full((nchunks + 1,), -77, dtype=torch.int64, device="cuda")
            rc = _lib.query_windows(_lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF, esz, batch.data.data_ptr(),
                                    batch.offsets.data_ptr(), nchunks, chunk_len, D, W, ops, 0,
                                    mn.data_ptr() if ops & 1 else None, mx.data_ptr() if ops & 2 else None,
                                    sm.data_ptr() if ops & 4 else None, rets.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            _lib.check(rc)
            torch.cuda.synchronize()
            r = rets.cpu().numpy()
            assert np.array_equal(r[:nchunks], [min(chunk_len, n - c * chunk_len) for c in range(nchunks)]) and r[nchunks] == -77
            for bit, buf, w in ((1, mn, want[0]), (2, mx, want[1]), (4, sm, want[2])):
                h = buf.cpu().numpy()
                if bit == 4:
                    assert np.all(h[m:] == 0x5A5A5A5A5A5A5A5A), (codec, D, W, ops, "sum padding")
                    h = h.view(np.uint64)
                else:
                    assert np.all(h[m:] == sent), (codec, D, W, ops, bit, "padding")
                if ops & bit:
                    assert np.array_equal(h[:m].astype(np.uint64), w.reshape(-1).astype(np.uint64)), (codec, D, W, ops, bit)
                else:
                    assert np.all(h[:m] == (0x5A5A5A5A5A5A5A5A if bit == 4 else sent)), (codec, D, W, ops, bit, "unselected written")


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [
    ("xff", 2, 8, 5120, 0),       # decode_fast
    ("delta", 1, 1, 1024, 0),     # decode_uni
    ("delta", 1, 80, 10240, 0),   # decode_fast, 2 columns a lane
    ("xff", 2, 8, 5120, 1),       # decode_kernel (NO_FAST)
])
def test_query_windows_damaged_chunk(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    import torch
    no_fast(fam)
    rng = np.random.default_rng(5)
    nchunks = 9
    n = nchunks * chunk_len - 100
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    bad = 4
    off = int(batch.offsets[bad].item())
    hdr = batch.data[off + 6:off + 8].clone()
    batch.data[off + 6] = hdr[0] ^ 0x5                  # the header's ndims field
    W = 32
    want = wm.chunk_windows(x, chunk_len, D, W)
    res = cd.query_windows(batch, W, per_chunk=True, check=False)
    rets = torch.empty(nchunks, dtype=torch.int64, device="cuda")
    from sprintz_amd import _lib
    _lib.check(_lib.query_windows(_lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF, esz, batch.data.data_ptr(),
                                  batch.offsets.data_ptr(), nchunks, chunk_len, D, W, 7, 0, res["min"].data_ptr(),
                                  res["max"].data_ptr(), res["sum"].data_ptr(), rets.data_ptr(),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    r = rets.cpu().numpy()
    assert r[bad] < 0
    assert all(r[c] == min(chunk_len, n - c * chunk_len) for c in range(nchunks) if c != bad)
    keep = np.arange(nchunks) != bad
    for k, w in zip(("min", "max", "sum"), want):
        g = res[k].cpu().numpy()
        g = g.view(np.uint64) if k == "sum" else g
        assert np.array_equal(g[keep].astype(np.uint64), w[keep].astype(np.uint64)), k
    with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):
        cd.query_windows(batch, W, per_chunk=True, check=True)
    batch.data[off + 6] = hdr[0]
    cd.query_windows(batch, W, per_chunk=True, check=True)     # repaired: no error


@pytest.mark.parametrize("codec,esz,D,chunk_len,W,n", [
    ("xff", 2, 8, 5120, 64, 5120 * 11 + 8 * 70),         # W divides R = 640, partial last window
    ("xff", 2, 8, 5120, 640, 5120 * 11 + 8 * 70),        # W = R
    ("delta", 1, 8, 4096, 2048, 4096 * 13 + 8 * 3 + 5),  # W = 4 R: the fold, partial last window and row
    ("delta", 1, 1, 1024, 3072, 1024 * 20 + 17),         # univariate, W = 3 R
    ("delta", 1, 80, 10240, 32, 10240 * 6 + 80 * 9),     # cfg3's shape
    ("delta", 2, 3, 300, 500, 300 * 12 + 2),             # R = 100 is no multiple of 8: one kernel window of 104 rows a chunk
    ("delta", 2, 3, 36, 12, 36 * 5 + 3 * 4 + 2),         # W = R = 12, no multiple of 8: one kernel window of 16 rows a chunk, nothing folds
    ("xff", 1, 5, 60, 12, 60 * 4 + 5 * 7 + 3),           # the same with five columns
])
def test_query_windows_global(sz, oracle, codec, esz, D, chunk_len, W, n):
    rng = np.random.default_rng(n)
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    got = cd.query_windows(batch, W, ops=("min", "max", "sum", "count", "mean"))
    want = wm.global_windows(x, D, W)
    for k in ("min", "max", "sum", "count"):
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape, k
        assert np.array_equal(g.astype(np.int64), want[k].astype(np.int64)), k
    assert got["min"].dtype == cd.dtype and got["max"].dtype == cd.dtype
    ok = want["count"] > 0
    assert np.array_equal(got["mean"].cpu().numpy()[ok], want["mean"][ok])
    sub = cd.query_windows(batch, W, ops=("max",))
    assert list(sub) == ["max"] and np.array_equal(sub["max"].cpu().numpy(), got["max"].cpu().numpy())


def test_query_windows_global_refuses_unaligned_shapes(sz):
    import torch
    cd = sz.ChunkedCodec("delta", 1, 80, 1024, device="cuda:0")
    x = torch.randint(0, 255, (1024 * 4,), dtype=torch.uint8, device="cuda:0")
    batch = cd.compress(x)
    with pytest.raises(ValueError):
        cd.query_windows(batch, 32)                     # 1 024 elements are no whole rows of 80
    res = cd.query_windows(batch, 8, per_chunk=True)    # per_chunk serves it
    assert res["min"].shape == (4, 2, 80)
    cd2 = sz.ChunkedCodec("xff", 2, 8, 640, device="cuda:0")
    b2 = cd2.compress(torch.randint(0, 60000, (640 * 3,), dtype=torch.int32, device="cuda:0").to(torch.uint16))
    with pytest.raises(ValueError):
        cd2.query_windows(b2, 24)                       # R = 80: neither a multiple nor a divisor of 24


@pytest.mark.parametrize("name,W", [("cfg2", 64), ("cfg3_10k", 32), ("cfg1", 64)])
def test_query_windows_bench_sizes(sz, name, W):
    """the bench's own inputs at full size: every entry equals torch's reductions of the device-decoded batch"""
    import torch
    from rowdata import bench_input
    (codec, esz, D, chunk_len, nchunks), x = bench_input(name, "cuda:0")
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device="cuda:0")
    batch = cd.compress(x)
    dec = cd.decompress(batch)
    got = cd.query_windows(batch, W, per_chunk=True)
    R = chunk_len // D
    v = dec.view(nchunks, R // W, W, D).to(torch.int32)
    assert torch.equal(got["min"].to(torch.int32), v.amin(dim=2))
    assert torch.equal(got["max"].to(torch.int32), v.amax(dim=2))
    assert torch.equal(got["sum"], v.to(torch.int64).sum(dim=2))
    del v, dec
