"""GPU tests (-m gpu) of aggregate rows (sprintz_mi355x_aggregate_rows, ChunkedCodec.aggregate_rows / aggregate_where): per-window
min / max / sum / count of the rows a mask names, fused into the decode, in decode_fast.h and decode_kernel.h.  The expected value is
always tests/aggregate_model.py applied to the ORIGINAL input -- decode is lossless and pinned elsewhere.  Every launch's kernel family
is asserted, every output lies in a sentinel-filled buffer whose padding must keep the sentinel, and rets[nchunks] must stay untouched.
Every batch ends in a short last chunk of whole rows."""
import zlib

import numpy as np
import pytest

import aggregate_model as am
import filter_model as fm
from dispatch import ran
from harness import DTYPES
from fixtures import no_fast, sz  # noqa: F401  (fixtures)
from rowdata import (FAST_SHAPES, PARITY_FAST, bound_sets, gen_data, lowdim, make_batch, masked_parity_cases as parity_cases, parity_masks, rows_for,
                     short_batch, windows_for)
from rowop_runners import check_agg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("codec,esz,D,shape,data", parity_cases())
def test_aggregate_rows_parity(sz, oracle, no_fast, codec, esz, D, shape, data):
    """both layouts of the low-dimension shapes x eleven masks x five windows x both families: every output equals the model"""
    rng = np.random.default_rng(zlib.crc32(f"aggregate{codec}{esz}{D}{shape}{data}".encode()))
    R = rows_for(shape, D)
    chunk_len = R * D
    x = gen_data(data, rng, short_batch(5, chunk_len, D), esz, D)
    masks = parity_masks(rng, x, chunk_len, esz, D)
    want = {(name, W): am.aggregate_rows(x, chunk_len, D, mask, W) for name, mask in masks for W in windows_for(R)}
    for general in ((False, True) if lowdim(esz, D) else (False,)):
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, general)
        first = "dec_fast" if (esz, D, general) in PARITY_FAST else "dec_generic"
        for fam, family in ((0, first), (1, "dec_generic")):
            if fam == 1 and first == "dec_generic":
                continue                                   # (the same kernel again)
            no_fast(fam)
            for name, mask in masks:
                for W in windows_for(R):
                    with ran(only=[family], **{family: 1}):
                        check_agg(x, batch, codec, esz, D, chunk_len, mask, W, (codec, esz, D, shape, data, general, family, name, W),
                                  want[(name, W)], general=general)
    assert int(want[("no row", 8)]["count"].sum()) == 0
    assert int(want[("every bit", 8)]["count"].sum()) == x.size // D and int(want[("row 0", 8)]["count"].sum()) == 5


@pytest.mark.parametrize("codec,esz,D,chunk_len", FAST_SHAPES)
def test_aggregate_rows_fast_mappings(sz, oracle, no_fast, codec, esz, D, chunk_len):
    """the parity matrix's chunks are too short for most of decode_fast.h's mappings: each of them, on chunks it takes, under the
    eleven masks at a window inside the chunk and at one window a chunk; the generic kernel on the same batch"""
    rng = np.random.default_rng(zlib.crc32(f"fast{codec}{esz}{D}".encode()))
    R = chunk_len // D
    x = gen_data("walk", rng, short_batch(4, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    masks = parity_masks(rng, x, chunk_len, esz, D)
    for W in (24, -(-R // 8) * 8):
        for name, mask in masks:
            want = None
            for fam, family in ((0, "dec_fast"), (1, "dec_generic")):
                no_fast(fam)
                with ran(only=[family], **{family: 1}):
                    want = check_agg(x, batch, codec, esz, D, chunk_len, mask, W, (codec, esz, D, family, name, W), want)


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam,family", [
    ("xff", 2, 8, 5120, 0, "dec_fast"),
    ("delta", 1, 80, 10240, 0, "dec_fast"),
    ("delta", 2, 12, 12 * 400, 0, "dec_fast"),    # (a reduce-only mode: rows need not be whole 16-byte pieces)
    ("delta", 1, 1, 1024, 0, "dec_generic"),
    ("xff", 1, 3, 3000, 0, "dec_generic"),
    ("delta", 2, 300, 9600, 0, "dec_generic"),
    ("xff", 2, 8, 5120, 1, "dec_generic"),
])
def test_aggregate_rows_each_op_alone(sz, oracle, no_fast, codec, esz, D, chunk_len, fam, family):
    """each op alone, pairs and all four, under two sentinels: an output that is not selected stays untouched -- given, or NULL"""
    no_fast(fam)
    rng = np.random.default_rng(D + fam)
    x = gen_data("walk", rng, short_batch(6, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    name, mode, lo, hi, _ = sets[0]
    mask, cnt = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
    assert 0 < int(cnt.sum()) < x.size // D
    for W in (64, -(-(chunk_len // D) // 8) * 8):
        want = am.aggregate_rows(x, chunk_len, D, mask, W)
        assert np.array_equal(want["count"].sum(axis=1), cnt)
        for ops, byte in ((1, 0x5A), (2, 0xA5), (4, 0x5A), (8, 0xA5), (15, 0x5A), (15, 0xA5), (9, 0x5A), (6, 0xA5)):
            for null in (False, True):
                with ran(only=[family], **{family: 1}):
                    check_agg(x, batch, codec, esz, D, chunk_len, mask, W, (codec, esz, D, family, W, ops, null), want, ops, byte, null_unselected=null)


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz,D", [(2, 8), (1, 16), (1, 3)])
def test_aggregate_rows_long_runs(sz, oracle, no_fast, codec, esz, D):
    """a constant batch and a batch that is flat for whole chunks (behind 40 rows of a walk: the run starts inside a window): runs of
    hundreds of blocks that cross many windows -- decode_fast.h's delta shortcut against the row loops -- under a mask of 3 rows of
    every 8, one of a single window, every row and none"""
    R = 2048
    chunk_len = D * R
    top = (1 << (8 * esz)) - 1
    rng = np.random.default_rng(esz + D)
    nchunks = 3
    rows = nchunks * R - 700
    const = np.full(rows * D, 0xA5 if esz == 1 else 0x1234, DTYPES[esz])
    flat = np.zeros((rows, D), np.int64)
    for c in range(nchunks):
        seg = flat[c * R:(c + 1) * R]
        seg[:] = rng.integers(2, top - 1, D)
        head = min(40, seg.shape[0])
        seg[:head] = np.mod(seg[:head] + np.cumsum(rng.integers(-3, 4, size=(head, D)), axis=0)[::-1], top + 1)
    flat = flat.astype(DTYPES[esz]).ravel()
    MB = R // 8
    kinds = {"3 of 8": np.full((nchunks, MB), 0b00100101, np.uint8), "one window": np.zeros((nchunks, MB), np.uint8),
             "every row": np.full((nchunks, MB), 0xFF, np.uint8), "no row": np.zeros((nchunks, MB), np.uint8)}
    kinds["one window"][:, 5 * 8:6 * 8] = 0xFF             # rows 320 .. 383: window 5 of 64 rows
    first = "dec_generic" if lowdim(esz, D) else "dec_fast"
    for label, x in (("constant", const), ("flat chunks", flat)):
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        for name, mask in kinds.items():
            for W in (64, 72, R):
                want = am.aggregate_rows(x, chunk_len, D, mask, W)
                for fam, family in ((0, first), (1, "dec_generic")):
                    no_fast(fam)
                    with ran(only=[family], **{family: 1}):
                        check_agg(x, batch, codec, esz, D, chunk_len, mask, W, (codec, esz, D, label, name, W, family), want)
                if name == "one window" and W == 64:
                    assert np.all(want["count"][:2, 5] == 64) and int(want["count"].sum()) == 64 * 3
                if name == "3 of 8" and label == "constant" and R % W == 0:
                    assert np.all(want["sum"][0] == np.uint64(int(const[0]) * 3 * (W // 8)))


@pytest.mark.parametrize("codec,esz,D,chunk_len,family", [
    ("xff", 2, 8, 8 * 650, "dec_fast"),           # R = 650: 2 rows in the last mask byte, MB = 82 is no multiple of 4, a verbatim tail of 10 rows
    ("delta", 1, 16, 16 * 203, "dec_fast"),       # R = 203, MB = 26
    ("delta", 2, 3, 3 * 333, "dec_generic"),      # (chunks of 1 998 bytes: no whole 16-byte pieces)
    ("xff", 1, 2, 2 * 1001, "dec_generic"),
])
def test_aggregate_rows_ignores_rows_that_do_not_exist(sz, oracle, no_fast, codec, esz, D, chunk_len, family):
    """every bit set -- on the short chunk's missing rows and on rows >= R in the last byte too -- counts and folds the existing rows
    alone; and the mask at an odd address with a short last dword (select's read-ahead window, byte by byte)"""
    rng = np.random.default_rng(chunk_len)
    R, MB = fm.geometry(chunk_len, D)
    assert R % 8 and MB % 4
    nchunks = 5
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    ones = np.full((nchunks, MB), 0xFF, np.uint8)
    clean = np.packbits(am.selected(ones, x.size, chunk_len, D), axis=1, bitorder="little")
    half = np.packbits(rng.random((nchunks, MB * 8)) < 0.5, axis=1, bitorder="little")
    for fam, fml in ((0, family), (1, "dec_generic")):
        no_fast(fam)
        for W in (8, 64, MB * 8):
            want = am.aggregate_rows(x, chunk_len, D, clean, W)
            assert int(want["count"].sum()) == x.size // D
            for shift in (0, 1, 3):
                with ran(only=[fml], **{fml: 2}):
                    check_agg(x, batch, codec, esz, D, chunk_len, ones, W, (codec, D, fml, W, shift, "every bit"), want, mask_shift=shift)
                    check_agg(x, batch, codec, esz, D, chunk_len, half, W, (codec, D, fml, W, shift, "p=1/2"), mask_shift=shift)


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [
    ("xff", 2, 8, 5120, 0),       # decode_fast
    ("delta", 1, 80, 10240, 0),   # decode_fast, two columns a lane
    ("xff", 2, 8, 5120, 1),       # decode_kernel (NO_FAST)
    ("delta", 1, 1, 1024, 0),     # decode_kernel, low-dimension layout
])
def test_aggregate_rows_damaged_chunk(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    import torch
    no_fast(fam)
    rng = np.random.default_rng(5)
    nchunks = 9
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    bad = 4
    off = int(batch.offsets[bad].item())
    hdr = batch.data[off + 6:off + 8].clone()
    R, MB = fm.geometry(chunk_len, D)
    mask = np.packbits(rng.random((nchunks, MB * 8)) < 0.4, axis=1, bitorder="little")
    mask_t = torch.from_numpy(mask).cuda()
    batch.data[off + 6] = hdr[0] ^ 0x5                  # the header's ndims field
    for W in (32, MB * 8):
        check_agg(x, batch, codec, esz, D, chunk_len, mask, W, (codec, D, fam, W), skip_chunk=bad)
    with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):
        cd.aggregate_rows(batch, mask_t, 32, per_chunk=True, check=True)
    cd.aggregate_rows(batch, mask_t, 32, per_chunk=True, check=False)      # no error without the check
    batch.data[off + 6] = hdr[0]
    got = cd.aggregate_rows(batch, mask_t, 32, per_chunk=True)             # repaired: no error, and exact
    want = am.aggregate_rows(x, chunk_len, D, mask, 32)
    for k in ("min", "max", "sum", "count"):
        assert np.array_equal(got[k].cpu().numpy().astype(np.uint64), want[k].astype(np.uint64)), k


@pytest.mark.parametrize("codec,esz,D,chunk_len,W,nchunks", [
    ("xff", 2, 8, 5120, 64, 6),            # W divides R = 640
    ("xff", 2, 8, 5120, 640, 6),           # W = R
    ("delta", 1, 8, 4096, 2048, 9),        # W = 4 R: the fold, with a partial last window
    ("delta", 1, 1, 1024, 3072, 10),       # univariate, W = 3 R
    ("delta", 2, 3, 300, 500, 12),         # R = 100 is no multiple of 8: one kernel window of 104 rows a chunk
])
def test_aggregate_rows_python_global_windows(sz, oracle, codec, esz, D, chunk_len, W, nchunks):
    import torch
    rng = np.random.default_rng(W + D)
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    R, MB = fm.geometry(chunk_len, D)
    bits = rng.random((nchunks, MB * 8)) < 0.3
    bits[nchunks // 2] = False                               # a chunk without a selected row: empty windows
    mask = np.packbits(bits, axis=1, bitorder="little")
    mask_t = torch.from_numpy(mask).cuda()
    got = cd.aggregate_rows(batch, mask_t, W, ops=("min", "max", "sum", "count", "mean"))
    want = am.global_windows(x, chunk_len, D, mask, W)
    for k in ("min", "max", "sum", "count"):
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape, k
        assert np.array_equal(g.astype(np.int64), want[k].astype(np.int64)), k
    assert got["min"].dtype == cd.dtype and got["max"].dtype == cd.dtype and got["sum"].dtype == torch.int64 and got["count"].dtype == torch.int64
    mean = got["mean"].cpu().numpy()
    empty = want["count"] == 0
    assert mean.dtype == np.float64 and np.all(np.isnan(mean[empty])) and np.array_equal(mean[~empty], want["mean"][~empty])
    if W <= R:
        assert empty.any()
    sub = cd.aggregate_rows(batch, mask_t, W, ops="max")
    assert list(sub) == ["max"] and torch.equal(sub["max"].view(torch.int8 if esz == 1 else torch.int16), got["max"].view(torch.int8 if esz == 1 else torch.int16))
    one = cd.aggregate_rows(batch, mask_t, per_chunk=True)                   # window_rows=None: one window a chunk
    want1 = am.aggregate_rows(x, chunk_len, D, mask, MB * 8)
    assert one["count"].shape == (nchunks, 1) and one["sum"].shape == (nchunks, 1, D)
    for k in ("min", "max", "sum", "count"):
        assert np.array_equal(one[k].cpu().numpy().astype(np.uint64), want1[k].astype(np.uint64)), k
    glob1 = cd.aggregate_rows(batch, mask_t)                                 # ... and as global windows of R rows
    assert np.array_equal(glob1["count"].cpu().numpy(), am.global_windows(x, chunk_len, D, mask, R)["count"])


def test_aggregate_where_python(sz, oracle):
    import torch
    codec, esz, D, chunk_len = "xff", 2, 8, 5120
    rng = np.random.default_rng(21)
    x = gen_data("walk", rng, short_batch(6, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    for name, mode, lo, hi, _ in sets[:2]:                 # the band (ALL) and the alarm (ANY)
        mask, cnt = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
        for W in (64, 640, 1280):
            with ran(only=["dec_fast"], dec_fast=2):       # the filter launch and the aggregate launch
                got = cd.aggregate_where(batch, list(map(int, lo)), list(map(int, hi)), mode="all" if mode == fm.ALL else "any", window_rows=W,
                                         ops=("count", "min", "max", "sum", "mean"))
            want = am.global_windows(x, chunk_len, D, mask, W)
            assert int(want["count"].sum()) == int(cnt.sum()) > 0
            for k in ("min", "max", "sum", "count"):
                assert np.array_equal(got[k].cpu().numpy().astype(np.int64), want[k].astype(np.int64)), (name, W, k)
            assert np.array_equal(got["mean"].cpu().numpy(), want["mean"], equal_nan=True), (name, W)
    none = cd.aggregate_where(batch, 1, 0)                 # an empty interval: no row, one window a chunk
    assert int(none["count"].sum().item()) == 0 and bool((none["sum"] == 0).all()) and none["count"].shape == (6,)
    f = cd.filter_rows(batch, 0, 65535)
    with pytest.raises(ValueError):
        cd.aggregate_rows(batch, f["mask"][:, :-1])
    with pytest.raises(ValueError):
        cd.aggregate_rows(batch, f["mask"], 24)            # R = 640: neither a multiple nor a divisor of 24
    with pytest.raises(ValueError):
        cd.aggregate_rows(batch, f["mask"], 64, ops=("median",))
    assert cd.aggregate_rows(batch, f["mask"], 24, per_chunk=True)["count"].shape == (6, 27)
    ragged = sz.ChunkedCodec("delta", 1, 80, 1024, device="cuda:0")        # 1 024 elements are no whole rows of 80
    rb = ragged.compress(torch.randint(0, 255, (1024 * 4,), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):
        ragged.aggregate_rows(rb, torch.zeros((4, 2), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):
        ragged.aggregate_where(rb, 0, 100)


def test_aggregate_rows_headline_shape(sz, oracle):
    """64 chunks of the headline shape (uint16 x 8, FIRE, 10 KB chunks), filter_rows' band mask from the device, W = 64"""
    codec, esz, D, chunk_len, nchunks, W = "xff", 2, 8, 5120, 64, 64
    rng = np.random.default_rng(64)
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    name, mode, lo, hi, _ = sets[0]
    f = cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)))
    mask = f["mask"].cpu().numpy()
    want_mask, cnt = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
    assert np.array_equal(mask, want_mask) and 0 < int(cnt.sum()) < x.size // D
    with ran(only=["dec_fast"], dec_fast=1):
        want = check_agg(x, batch, codec, esz, D, chunk_len, mask, W, ("headline",))
    assert np.array_equal(want["count"].sum(axis=1), cnt)
    with ran(only=["dec_fast"], dec_fast=1):
        got = cd.aggregate_rows(batch, f["mask"], W, per_chunk=True)
    for k in ("min", "max", "sum", "count"):
        assert np.array_equal(got[k].cpu().numpy().astype(np.uint64), want[k].astype(np.uint64)), k
