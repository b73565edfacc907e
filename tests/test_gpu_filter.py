"""GPU tests (-m gpu) of filter rows (sprintz_mi355x_filter_rows / _filter_row_ids, ChunkedCodec.filter_rows): row predicates fused
into the three decoder families (decode_fast.h, decode_uni.h, decode_kernel.h).  The expected value is always tests/filter_model.py
applied to the ORIGINAL input -- decode is lossless and pinned elsewhere."""
import ctypes as C
import zlib

import numpy as np
import pytest

import filter_model as fm
from dispatch import ran
from harness import DTYPES
from fixtures import no_fast, sz  # noqa: F401  (fixtures)
from rowdata import bound_sets, chunk_len_for, gen_data, make_batch, parity_cases
from rowop_runners import run_filter

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("codec,esz,D,shape,data,general", parity_cases())
def test_filter_rows_parity(sz, oracle, no_fast, codec, esz, D, shape, data, general):
    """the matrix of test_gpu_query_windows.py (same seeds, same batches) x both families x six bound sets: mask and counts equal the model"""
    rng = np.random.default_rng(zlib.crc32(f"{codec}{esz}{D}{shape}{data}{general}".encode()))
    chunk_len = chunk_len_for(shape, D)
    nchunks = 5 + D % 4
    n = nchunks * chunk_len - chunk_len // 3 - 1          # every batch ends in a short last chunk
    x = gen_data(data, rng, n, esz, D)
    sets, nrows = bound_sets(x, chunk_len, esz, D)
    want = {}
    for name, mode, lo, hi, expect in sets:
        want[name] = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
        total = int(want[name][1].sum())
        if expect == "all":
            assert total == nrows, name
        elif expect == "none":
            assert total == 0, name
        elif name == "band" and data in ("walk", "uniform", "sparse"):
            assert 0 < total < nrows, (name, total, nrows)
        elif name == "alarm" and data in ("walk", "uniform"):
            assert 0 < total < nrows, (name, total, nrows)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, general)
    for fam in (0, 1):
        no_fast(fam)
        for name, mode, lo, hi, _ in sets:
            mask, counts = run_filter(cd, batch, lo, hi, mode, general)
            msg = (codec, esz, D, shape, data, general, fam, name)
            assert mask.shape == want[name][0].shape, msg
            assert np.array_equal(counts, want[name][1]), ("counts",) + msg
            assert np.array_equal(mask, want[name][0]), ("mask",) + msg


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam,family", [
    ("xff", 2, 8, 5120, 0, "dec_fast"),
    ("delta", 1, 80, 10240, 0, "dec_fast"),       # two columns a lane
    ("delta", 1, 1, 1024, 0, "dec_uni"),
    ("delta", 2, 300, 9600, 0, "dec_generic"),    # more than 256 columns
    ("xff", 2, 8, 5120, 1, "dec_generic"),        # any shape under OPT_NO_FAST
    ("delta", 1, 1, 1024, 1, "dec_generic"),
])
def test_filter_rows_which_kernel(sz, oracle, no_fast, codec, esz, D, chunk_len, fam, family):
    no_fast(fam)
    rng = np.random.default_rng(D + fam)
    n = 6 * chunk_len - 7 * D - (3 if D > 1 else 0)
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    name, mode, lo, hi, _ = sets[0]
    with ran(only=[family], **{family: 1}):
        mask, counts = run_filter(cd, batch, lo, hi, mode)
    want = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
    assert np.array_equal(mask, want[0]) and np.array_equal(counts, want[1])


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz", [1, 2])
def test_filter_rows_long_runs(sz, oracle, no_fast, codec, esz):
    """flat spans of 3 200 rows inside a chunk: runs of 400 blocks (a two-byte run length), which the delta filter never replays row
    by row; bounds the flat value satisfies, and bounds it misses by one"""
    D, R = 8, 4096
    chunk_len = D * R
    top = (1 << (8 * esz)) - 1
    rng = np.random.default_rng(esz)
    nchunks = 3
    rows = nchunks * R - 700
    steps = rng.integers(-3, 4, size=(rows, D))
    x = np.mod(np.cumsum(steps, axis=0) + rng.integers(0, top, size=(1, D)), top + 1)
    flat = rng.integers(2, top - 1, D)
    for c in range(nchunks):
        x[c * R + 500:c * R + 3700] = flat                 # (the last chunk's span is cut short by the batch's end)
    x = x.astype(DTYPES[esz]).ravel()
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    never = (np.full(D, top), np.zeros(D, np.int64))
    always = (np.zeros(D, np.int64), np.full(D, top))
    sets = [("hit", fm.ALL, flat.copy(), flat.copy())]
    for d in (0, D - 1):
        lo, hi = flat.copy(), flat.copy()
        lo[d] += 1
        hi[d] = top
        sets.append((f"above {d}", fm.ALL, lo, hi))        # misses the flat value by one
        lo, hi = flat.copy(), flat.copy()
        lo[d], hi[d] = 0, flat[d] - 1
        sets.append((f"below {d}", fm.ALL, lo, hi))
        lo, hi = never[0].copy(), never[1].copy()
        lo[d], hi[d] = flat[d], flat[d]
        sets.append((f"any hit {d}", fm.ANY, lo, hi))
        lo, hi = never[0].copy(), never[1].copy()
        lo[d], hi[d] = flat[d] + 1, top
        sets.append((f"any above {d}", fm.ANY, lo, hi))
    sets.append(("always", fm.ALL) + always)
    for fam in (0, 1):
        no_fast(fam)
        for name, mode, lo, hi in sets:
            want = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
            if name == "hit":
                assert want[1][0] >= 3200
            mask, counts = run_filter(cd, batch, lo, hi, mode)
            assert np.array_equal(counts, want[1]), (codec, esz, fam, name, counts, want[1])
            assert np.array_equal(mask, want[0]), (codec, esz, fam, name)


GUARD_SHAPES = [
    ("xff", 2, 8, 5120),          # decode_fast
    ("delta", 1, 1, 1024),        # decode_uni
    ("xff", 1, 3, 3001),          # decode_uni, 3 columns, ragged
    ("delta", 2, 300, 9677),      # decode_kernel
]


@pytest.mark.parametrize("codec,esz,D,chunk_len", GUARD_SHAPES)
def test_filter_rows_output_guards(sz, oracle, codec, esz, D, chunk_len):
    """sentinel-filled, padded outputs: nothing lands past nchunks*MB / nchunks, every byte inside is written, either output may be NULL"""
    import torch
    from sprintz_amd import _lib
    rng = np.random.default_rng(D)
    nchunks = 7
    n = nchunks * chunk_len - chunk_len // 2
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    R, MB = fm.geometry(chunk_len, D)
    pad = 4096
    dt = torch.uint8 if esz == 1 else torch.uint16
    for name, mode, lo, hi, _ in sets[:3]:
        want = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
        lo_t = torch.from_numpy(lo.astype(np.int32)).cuda().to(dt)
        hi_t = torch.from_numpy(hi.astype(np.int32)).cuda().to(dt)
        for sent in (0x5A, 0xA5):                          # two sentinels: a byte that equals one of them by value was still written
            for outs in ("both", "mask", "counts"):
                mask = torch.full((nchunks * MB + pad,), sent, dtype=torch.uint8, device="cuda")
                counts = torch.full((nchunks + 64,), -77, dtype=torch.int32, device="cuda")
                rets = torch.full((nchunks + 1,), -77, dtype=torch.int64, device="cuda")
                rc = _lib.filter_rows(_lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF, esz, batch.data.data_ptr(),
                                      batch.offsets.data_ptr(), nchunks, chunk_len, D, lo_t.data_ptr(), hi_t.data_ptr(), mode, 0,
                                      mask.data_ptr() if outs != "counts" else None, counts.data_ptr() if outs != "mask" else None,
                                      rets.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
                _lib.check(rc)
                torch.cuda.synchronize()
                r = rets.cpu().numpy()
                assert np.array_equal(r[:nchunks], [min(chunk_len, n - c * chunk_len) for c in range(nchunks)]) and r[nchunks] == -77
                m, k = mask.cpu().numpy(), counts.cpu().numpy()
                assert np.all(m[nchunks * MB:] == sent) and np.all(k[nchunks:] == -77), (codec, D, name, outs, "padding")
                if outs != "counts":
                    assert np.array_equal(m[:nchunks * MB].reshape(nchunks, MB), want[0]), (codec, D, name, outs, sent)
                else:
                    assert np.all(m == sent), "a NULL mask was written"
                if outs != "mask":
                    assert np.array_equal(k[:nchunks], want[1]), (codec, D, name, outs)
                else:
                    assert np.all(k == -77), "NULL counts were written"


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [
    ("xff", 2, 8, 5120, 0),       # decode_fast
    ("delta", 1, 1, 1024, 0),     # decode_uni
    ("delta", 1, 80, 10240, 0),   # decode_fast, 2 columns a lane
    ("xff", 2, 8, 5120, 1),       # decode_kernel (NO_FAST)
])
def test_filter_rows_damaged_chunk(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    import torch
    from sprintz_amd import _lib
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
    sets, _ = bound_sets(x, chunk_len, esz, D)
    name, mode, lo, hi, _ = sets[0]
    want = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
    R, MB = fm.geometry(chunk_len, D)
    dt = torch.uint8 if esz == 1 else torch.uint16
    lo_t = torch.from_numpy(lo.astype(np.int32)).cuda().to(dt)
    hi_t = torch.from_numpy(hi.astype(np.int32)).cuda().to(dt)
    mask = torch.full((nchunks * MB + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    counts = torch.full((nchunks + 8,), -77, dtype=torch.int32, device="cuda")
    rets = torch.empty(nchunks, dtype=torch.int64, device="cuda")
    _lib.check(_lib.filter_rows(_lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF, esz, batch.data.data_ptr(), batch.offsets.data_ptr(),
                                nchunks, chunk_len, D, lo_t.data_ptr(), hi_t.data_ptr(), mode, 0, mask.data_ptr(), counts.data_ptr(),
                                rets.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    r = rets.cpu().numpy()
    assert r[bad] < 0
    assert all(r[c] == min(chunk_len, n - c * chunk_len) for c in range(nchunks) if c != bad)
    keep = np.arange(nchunks) != bad
    m, k = mask.cpu().numpy(), counts.cpu().numpy()
    assert np.all(m[nchunks * MB:] == 0x5A) and np.all(k[nchunks:] == -77)        # nothing outside the outputs
    assert np.array_equal(m[:nchunks * MB].reshape(nchunks, MB)[keep], want[0][keep])
    assert np.array_equal(k[:nchunks][keep], want[1][keep])
    with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):
        cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), check=True)
    cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), check=False)    # no error without the check
    with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):                   # ... but ids are sized and placed by the counts: they check
        cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), ids=True, check=False)
    batch.data[off + 6] = hdr[0]
    got = cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), check=True)   # repaired: no error, and exact
    assert np.array_equal(got["mask"].cpu().numpy(), want[0]) and np.array_equal(got["counts"].cpu().numpy(), want[1])


@pytest.mark.parametrize("codec,esz,D,chunk_len", [
    ("xff", 2, 8, 5120),          # R = 640: 20 mask dwords a chunk
    ("delta", 1, 80, 10240),      # R = 128
    ("delta", 2, 3, 300),         # R = 100: 13 mask bytes, the last one partly padding, chunks start at odd mask addresses
    ("delta", 1, 1, 32768),       # 1 024 mask dwords a chunk: 16 trips of a 64-lane group
    ("xff", 1, 4, 4 * 20),        # R = 20: fewer mask dwords than the smallest group
])
def test_filter_row_ids(sz, oracle, codec, esz, D, chunk_len):
    import torch
    from sprintz_amd import _lib
    rng = np.random.default_rng(chunk_len)
    R = chunk_len // D
    nchunks = 6
    n = nchunks * chunk_len - (R // 3) * D                 # a short last chunk of whole rows
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, nrows = bound_sets(x, chunk_len, esz, D)
    rows = x.reshape(-1, D)
    for name, mode, lo, hi, expect in sets[:4]:             # band, alarm, all rows, no row (the empty result)
        want_mask, want_counts = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
        ok = (rows >= lo) & (rows <= hi)
        want = np.flatnonzero(ok.all(axis=1) if mode == fm.ALL else ok.any(axis=1))
        assert np.array_equal(fm.row_ids(want_mask, chunk_len, D), want)
        got = cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), mode="all" if mode == fm.ALL else "any", ids=True)
        ids = got["ids"]
        assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), want), (codec, D, name)
        if expect == "none":
            assert ids.numel() == 0
            continue
        # ids -> gather_rows(ids, 1) returns exactly the matching rows
        fetched = cd.gather_rows(batch, ids, 1)
        assert np.array_equal(fetched.cpu().numpy().reshape(-1, D), rows[want]), (codec, D, name)
        # a capacity below the total leaves the sentinel behind the cut, and nothing lands behind the array
        total = want.size
        cap = total // 2
        buf = torch.full((total + 32,), -9, dtype=torch.int64, device="cuda")
        bases = (torch.cumsum(got["counts"].to(torch.int64), 0) - got["counts"]).contiguous()
        _lib.check(_lib.filter_row_ids(got["mask"].data_ptr(), bases.data_ptr(), nchunks, chunk_len, D, buf.data_ptr(), cap,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        b = buf.cpu().numpy()
        assert np.array_equal(b[:cap], want[:cap]) and np.all(b[cap:] == -9), (codec, D, name, "capacity")


def test_filter_row_ids_need_whole_rows(sz):
    import torch
    cd = sz.ChunkedCodec("delta", 1, 80, 1024, device="cuda:0")            # 1 024 elements are no whole rows of 80
    batch = cd.compress(torch.randint(0, 255, (1024 * 4,), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):
        cd.filter_rows(batch, 0, 100, ids=True)
    res = cd.filter_rows(batch, 0, 255)                                     # the mask alone serves it: 12 whole rows a chunk
    assert res["mask"].shape == (4, 2) and res["counts"].tolist() == [12] * 4


def test_filter_rows_python_bounds(sz, oracle):
    """scalars, sequences with None entries and device tensors describe the same bounds"""
    import torch
    esz, D, chunk_len = 2, 8, 5120
    rng = np.random.default_rng(11)
    x = gen_data("uniform", rng, 4 * chunk_len - 24, esz, D)
    cd, batch = make_batch(sz, oracle, "xff", esz, D, chunk_len, x, False)
    top = 0xFFFF
    lo = [None, 1000, None, None, None, None, None, 30000]
    hi = [None, None, None, 50000, None, None, None, 40000]
    for mode, m in (("all", fm.ALL), ("any", fm.ANY)):
        nlo, nhi = fm.neutral(esz, m)
        wlo = [(nlo if (a is None and b is None) else 0) if a is None else a for a, b in zip(lo, hi)]
        whi = [(nhi if (a is None and b is None) else top) if b is None else b for a, b in zip(lo, hi)]
        want = fm.filter_rows(x, chunk_len, D, wlo, whi, m)
        got = cd.filter_rows(batch, lo, hi, mode=mode)
        assert np.array_equal(got["mask"].cpu().numpy(), want[0]) and np.array_equal(got["counts"].cpu().numpy(), want[1]), mode
        lo_t = torch.tensor(wlo, dtype=torch.int32, device="cuda").to(torch.uint16)
        hi_t = torch.tensor(whi, dtype=torch.int32, device="cuda").to(torch.uint16)
        got = cd.filter_rows(batch, lo_t, hi_t, mode=mode)
        assert np.array_equal(got["mask"].cpu().numpy(), want[0]), mode
    want = fm.filter_rows(x, chunk_len, D, [20000] * D, [60000] * D, fm.ANY)
    got = cd.filter_rows(batch, 20000, 60000, mode="any")
    assert np.array_equal(got["mask"].cpu().numpy(), want[0]) and got["counts"].dtype == torch.int32 and got["mask"].shape == (4, 80)
    with pytest.raises(ValueError):
        cd.filter_rows(batch, [0] * 7, 5)
    with pytest.raises(ValueError):
        cd.filter_rows(batch, 0, 70000)
    with pytest.raises(ValueError):
        cd.filter_rows(batch, 0, 5, mode="some")


def test_filter_rows_bench_size(sz):
    """the bench's headline input at full size, once: the band set against torch's comparison of the device-decoded batch"""
    import torch
    from rowdata import bench_input
    (codec, esz, D, chunk_len, nchunks), x = bench_input("cfg2", "cuda:0")
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device="cuda:0")
    batch = cd.compress(x)
    dec = cd.decompress(batch).view(-1, D)
    R = chunk_len // D
    top = (1 << (8 * esz)) - 1
    lo, hi = [0] * D, [top] * D
    for d in (0, D - 1):
        col = dec[:, d].to(torch.int32)
        nn = col.numel()
        lo[d] = int(torch.kthvalue(col, int(0.25 * (nn - 1)) + 1).values.item())     # the lower quantiles
        hi[d] = int(torch.kthvalue(col, int(0.75 * (nn - 1)) + 1).values.item())
        del col
    with ran(dec_fast=1):
        got = cd.filter_rows(batch, lo, hi, mode="all")
    ok = torch.ones(dec.shape[0], dtype=torch.bool, device="cuda:0")
    for d in (0, D - 1):
        col = dec[:, d].to(torch.int32)
        ok &= (col >= lo[d]) & (col <= hi[d])
        del col
    total = int(ok.sum().item())
    assert 0 < total < ok.numel()
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device="cuda:0")
    packed = (ok.view(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8)
    assert torch.equal(got["mask"].view(-1), packed)       # chunk_len % D == 0 and R % 8 == 0: the batch's rows in order
    assert torch.equal(got["counts"].to(torch.int64), ok.view(nchunks, R).sum(dim=1))
    assert int(got["counts"].sum().item()) == total
