"""GPU tests (-m gpu) of extrema rows (sprintz_mi355x_extrema_rows, ChunkedCodec.extrema_rows / extrema_where / m4): per-window
min / max with the rows they stand in, the first and the last selected sample, their rows and the count, fused into the decode, in
decode_fast.h and decode_kernel.h.  The expected value is always tests/extrema_model.py applied to the ORIGINAL input -- decode is
lossless and pinned elsewhere.  Every launch's kernel family is asserted, every output lies in a sentinel-filled buffer whose padding
must keep the sentinel, and rets[nchunks] must stay untouched.  Every batch ends in a short last chunk of whole rows.  The kernels keep
value and row apart: there is no window limit, so no position edge to drive."""
import zlib

import numpy as np
import pytest

import extrema_model as em
import filter_model as fm
from dispatch import ran
from harness import DTYPES
from fixtures import no_fast, sz  # noqa: F401  (fixtures)
from rowdata import (FAST_SHAPES, PARITY_FAST, bound_sets, gen_data, lowdim, make_batch, masked_parity_cases as parity_cases, parity_masks, rows_for,
                     short_batch, windows_for)
from rowop_runners import OUTS, check_ext

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("codec,esz,D,shape,data", parity_cases())
def test_extrema_rows_parity(sz, oracle, no_fast, codec, esz, D, shape, data):
    """both layouts of the low-dimension shapes x the eleven masks and the NULL mask x five windows x both families"""
    rng = np.random.default_rng(zlib.crc32(f"extrema{codec}{esz}{D}{shape}{data}".encode()))
    R = rows_for(shape, D)
    chunk_len = R * D
    x = gen_data(data, rng, short_batch(5, chunk_len, D), esz, D)
    masks = parity_masks(rng, x, chunk_len, esz, D) + [("null", None)]
    assert len(masks) == 12
    want = {(name, W): em.extrema_rows(x, chunk_len, D, mask, W) for name, mask in masks for W in windows_for(R)}
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
                        check_ext(x, batch, codec, esz, D, chunk_len, mask, W, (codec, esz, D, shape, data, general, family, name, W),
                                  want[(name, W)], general=general)
    assert int(want[("no row", 8)]["count"].sum()) == 0 and np.all(want[("no row", 8)]["rows"] == em.NO_ROW)
    assert int(want[("every bit", 8)]["count"].sum()) == x.size // D == int(want[("null", 8)]["count"].sum())
    for k in OUTS:
        assert np.array_equal(want[("every bit", 24)][k], want[("null", 24)][k])


@pytest.mark.parametrize("codec,esz,D,chunk_len", FAST_SHAPES)
def test_extrema_rows_fast_mappings(sz, oracle, no_fast, codec, esz, D, chunk_len):
    """each of decode_fast.h's lane mappings, on chunks it takes, under the twelve masks at a window inside the chunk and at one window
    a chunk; the generic kernel on the same batch"""
    rng = np.random.default_rng(zlib.crc32(f"extfast{codec}{esz}{D}".encode()))
    R = chunk_len // D
    x = gen_data("walk", rng, short_batch(4, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    masks = parity_masks(rng, x, chunk_len, esz, D) + [("null", None)]
    for W in (24, -(-R // 8) * 8):
        for name, mask in masks:
            want = None
            for fam, family in ((0, "dec_fast"), (1, "dec_generic")):
                no_fast(fam)
                with ran(only=[family], **{family: 1}):
                    want = check_ext(x, batch, codec, esz, D, chunk_len, mask, W, (codec, esz, D, family, name, W), want)


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam,family", [
    ("xff", 2, 8, 5120, 0, "dec_fast"),
    ("delta", 1, 80, 10240, 0, "dec_fast"),
    ("delta", 1, 1, 1024, 0, "dec_generic"),
    ("delta", 2, 300, 9600, 0, "dec_generic"),
    ("xff", 2, 8, 5120, 1, "dec_generic"),
])
def test_extrema_rows_each_op_alone(sz, oracle, no_fast, codec, esz, D, chunk_len, fam, family):
    """each op alone, the two families of pairs and all eight, under two sentinels: an output that is not selected stays untouched --
    given, or NULL; argmin without min is served"""
    no_fast(fam)
    rng = np.random.default_rng(D + fam)
    x = gen_data("walk", rng, short_batch(4, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    name, mode, lo, hi, _ = sets[0]
    mask, cnt = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
    assert 0 < int(cnt.sum()) < x.size // D
    W = 64
    want = em.extrema_rows(x, chunk_len, D, mask, W)
    assert np.array_equal(want["count"].sum(axis=1), cnt)
    for j, ops in enumerate((1, 2, 4, 8, 16, 32, 64, 128, 255, 4 | 8, 16 | 32 | 64)):
        for byte in (0x5A, 0xA5):
            null = (j + (byte == 0xA5)) % 2 == 1
            with ran(only=[family], **{family: 1}):
                check_ext(x, batch, codec, esz, D, chunk_len, mask, W, (codec, esz, D, family, ops, byte, null), want, ops, byte, null_unselected=null)


def edge_extremes(rng, esz, D, R, W, nchunks):
    """a batch whose minimum sits in row 0 and again in the last row of every window of W rows, and the same for the maximum: the first
    occurrence is the window's first row, whatever the later ones hold"""
    top = (1 << (8 * esz)) - 1
    x = rng.integers(top // 4, top // 2, (nchunks * R, D))
    for r in range(nchunks * R):
        if (r % R) % W in (0, W - 1) or r % R == R - 1:
            x[r, 0::2] = 1                                 # the even columns' minimum ...
            x[r, 1::2] = top - 1                           # ... and the odd columns' maximum
    return x.astype(DTYPES[esz])


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz,D", [(2, 8), (1, 16), (1, 3)])
def test_extrema_rows_ties_and_runs(sz, oracle, no_fast, codec, esz, D):
    """a constant batch and a batch that is flat for whole chunks (behind 40 rows of a walk: the run starts inside a window): runs of
    hundreds of blocks that cross many windows -- decode_fast.h's delta shortcut, its first and last selected row, a window the run
    leaves empty -- against the row loops, under a mask of 3 rows of every 8, one of a single window, every row, none and NULL; every
    position of a constant window is its first selected row"""
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
             "every row": np.full((nchunks, MB), 0xFF, np.uint8), "no row": np.zeros((nchunks, MB), np.uint8), "null": None}
    kinds["one window"][:, 5 * 8:6 * 8] = 0xFF             # rows 320 .. 383: window 5 of 64 rows
    kinds["one window"][:, 100] = 0x40                     # ... and row 806 alone, in window 12: the run's first selected row is its last
    first = "dec_generic" if lowdim(esz, D) else "dec_fast"
    edges = edge_extremes(rng, esz, D, R, 64, nchunks)[:rows].ravel()
    for label, x in (("constant", const), ("flat chunks", flat), ("extremes at the edges", edges)):
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        for name, mask in kinds.items():
            for W in (64, 72, R):
                want = em.extrema_rows(x, chunk_len, D, mask, W)
                for fam, family in ((0, first), (1, "dec_generic")):
                    no_fast(fam)
                    with ran(only=[family], **{family: 1}):
                        check_ext(x, batch, codec, esz, D, chunk_len, mask, W, (codec, esz, D, label, name, W, family), want)
                if label == "constant":
                    assert np.array_equal(want["argmin"], np.repeat(want["rows"][..., :1], D, axis=2)) and np.array_equal(want["argmin"], want["argmax"])
                if label == "constant" and name == "3 of 8" and W == 64:
                    assert want["rows"][0, 1].tolist() == [64, 64 + 61] and want["count"][0, 1] == 24
                if label == "extremes at the edges" and name in ("every row", "null") and W == 64:
                    starts = np.arange(R // 64) * 64                             # the first occurrence: row 0 of the window, not its last row
                    assert np.array_equal(want["argmin"][0, :, 0], starts) and np.array_equal(want["argmax"][0, :, 1], starts)


@pytest.mark.parametrize("codec,esz,D,chunk_len,family", [
    ("xff", 2, 8, 8 * 650, "dec_fast"),           # R = 650: 2 rows in the last mask byte, MB = 82 is no multiple of 4, a verbatim tail of 10 rows
    ("delta", 1, 16, 16 * 203, "dec_fast"),       # R = 203, MB = 26
    ("delta", 2, 3, 3 * 333, "dec_generic"),      # (chunks of 1 998 bytes: no whole 16-byte pieces)
    ("xff", 1, 2, 2 * 1001, "dec_generic"),
])
def test_extrema_rows_ignores_rows_that_do_not_exist(sz, oracle, no_fast, codec, esz, D, chunk_len, family):
    """every bit set -- on the short chunk's missing rows and on rows >= R in the last byte too -- takes the existing rows alone (the
    last row is the last EXISTING row); and the mask at an odd address with a short last dword"""
    rng = np.random.default_rng(chunk_len)
    R, MB = fm.geometry(chunk_len, D)
    assert R % 8 and MB % 4
    nchunks = 5
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    ones = np.full((nchunks, MB), 0xFF, np.uint8)
    half = np.packbits(rng.random((nchunks, MB * 8)) < 0.5, axis=1, bitorder="little")
    for fam, fml in ((0, family), (1, "dec_generic")):
        no_fast(fam)
        for W in (8, 64, MB * 8):
            want = em.extrema_rows(x, chunk_len, D, None, W)
            assert int(want["count"].sum()) == x.size // D and want["rows"][-1].max(initial=0, where=want["rows"][-1] != em.NO_ROW) == fm.chunk_counts(x.size, chunk_len)[-1] // D - 1
            for shift in (0, 1, 3):
                with ran(only=[fml], **{fml: 2}):
                    check_ext(x, batch, codec, esz, D, chunk_len, ones, W, (codec, D, fml, W, shift, "every bit"), want, mask_shift=shift)
                    check_ext(x, batch, codec, esz, D, chunk_len, half, W, (codec, D, fml, W, shift, "p=1/2"), mask_shift=shift)


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [
    ("xff", 2, 8, 5120, 0),       # decode_fast
    ("delta", 1, 80, 10240, 0),   # decode_fast, two columns a lane
    ("xff", 2, 8, 5120, 1),       # decode_kernel (NO_FAST)
    ("delta", 1, 1, 1024, 0),     # decode_kernel, low-dimension layout
])
def test_extrema_rows_damaged_chunk(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    """one stream of a 4-chunk batch truncated: its rets is negative, every other chunk's entries are exact, nothing outside is written"""
    import torch
    no_fast(fam)
    rng = np.random.default_rng(5)
    nchunks = 4
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    bad = 2
    R, MB = fm.geometry(chunk_len, D)
    mask = np.packbits(rng.random((nchunks, MB * 8)) < 0.4, axis=1, bitorder="little")
    mask_t = torch.from_numpy(mask).cuda()
    # chunk `bad`'s stream cut short by 5 bytes and the streams packed densely again, as test_gpu_parity.py truncates them
    comp0, offs, sizes = batch.data.cpu().numpy().copy(), batch.offsets.cpu().numpy(), batch.sizes.cpu().numpy()
    parts = [comp0[offs[c]:offs[c] + sizes[c] - (5 if c == bad else 0)] for c in range(nchunks)]
    toffs = np.zeros(nchunks + 1, np.int64)
    toffs[1:] = np.cumsum([p.size for p in parts])
    cut = type("Batch", (), {})()
    cut.nchunks = nchunks
    cut.data = torch.from_numpy(np.concatenate(parts + [np.zeros(sz._lib.READ_SLACK, np.uint8)])).cuda()
    cut.offsets = torch.from_numpy(toffs).cuda()
    for W in (32, MB * 8):
        check_ext(x, cut, codec, esz, D, chunk_len, mask, W, (codec, D, fam, W), skip_chunk=bad)
        check_ext(x, cut, codec, esz, D, chunk_len, None, W, (codec, D, fam, W, "null"), skip_chunk=bad)
    got = cd.extrema_rows(batch, mask_t, 32, per_chunk=True, ops=OUTS)       # the intact batch: no error, and exact
    want = em.extrema_rows(x, chunk_len, D, mask, 32)
    assert np.array_equal(got["count"].cpu().numpy(), want["count"])
    off = int(batch.offsets[bad].item())
    keep = batch.data[off + 6].clone()
    batch.data[off + 6] = keep ^ 0x5                        # the header's ndims field
    with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):
        cd.extrema_rows(batch, mask_t, 32, per_chunk=True, check=True)
    cd.extrema_rows(batch, mask_t, 32, per_chunk=True, check=False)          # no error without the check
    batch.data[off + 6] = keep


def to_np(t, esz):
    import torch
    if t.dtype in (torch.uint8, torch.uint16):
        return t.cpu().view(torch.int8 if esz == 1 else torch.int16).numpy().view(DTYPES[esz])
    return t.cpu().numpy()


@pytest.mark.parametrize("codec,esz,D,chunk_len,W,nchunks", [
    ("xff", 2, 8, 5120, 64, 6),            # W divides R = 640: fold 1
    ("xff", 2, 8, 5120, 640, 6),           # W = R: fold 1
    ("xff", 2, 8, 5120, 1280, 5),          # W = 2 R: fold 2, with a partial last window
    ("delta", 1, 8, 4096, 1024, 5),        # fold 2
    ("delta", 2, 3, 300, 200, 5),          # R = 100 is no multiple of 8: one kernel window of 104 rows a chunk, fold 2
])
def test_extrema_rows_python_global_windows(sz, oracle, codec, esz, D, chunk_len, W, nchunks):
    import torch
    rng = np.random.default_rng(W + D)
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    R, MB = fm.geometry(chunk_len, D)
    bits = rng.random((nchunks, MB * 8)) < 0.3
    bits[nchunks // 2] = False                               # a chunk without a selected row
    mask = np.packbits(bits, axis=1, bitorder="little")
    mask_t = torch.from_numpy(mask).cuda()
    for m_np, m_t in ((mask, mask_t), (None, None)):
        got = cd.extrema_rows(batch, m_t, W, ops=OUTS)
        want = em.global_windows(x, chunk_len, D, m_np, W)
        assert set(got) == set(want)
        for k, v in want.items():
            g = to_np(got[k], esz)
            assert g.shape == v.shape and g.dtype == v.dtype and np.array_equal(g, v), k
    assert got["argmin"].dtype == torch.int64 and got["min"].dtype == cd.dtype
    sub = cd.extrema_rows(batch, mask_t, W)                                   # the default ops; argmin alone asks the kernel for what the fold needs
    assert set(sub) == {"min", "argmin", "max", "argmax"}
    only = cd.extrema_rows(batch, mask_t, W, ops="argmin")
    want = em.global_windows(x, chunk_len, D, mask, W)
    assert list(only) == ["argmin"] and np.array_equal(only["argmin"].cpu().numpy(), want["argmin"]) and np.array_equal(sub["argmax"].cpu().numpy(), want["argmax"])
    ends = cd.extrema_rows(batch, mask_t, W, ops=("last", "rows"))
    assert set(ends) == {"last", "first_row", "last_row"} and np.array_equal(to_np(ends["last"], esz), want["last"])
    one = cd.extrema_rows(batch, mask_t, per_chunk=True, ops=OUTS)           # window_rows=None: one window a chunk, batch rows
    want1 = em.extrema_rows(x, chunk_len, D, mask, MB * 8)
    base = (np.arange(nchunks, dtype=np.int64) * R).reshape(-1, 1, 1)
    assert one["argmax"].shape == (nchunks, 1, D)
    assert np.array_equal(one["argmax"].cpu().numpy(), np.where(want1["argmax"] == em.NO_ROW, -1, want1["argmax"].astype(np.int64) + base))
    assert np.array_equal(one["last_row"].cpu().numpy(), np.where(want1["rows"][..., 1] == em.NO_ROW, -1, want1["rows"][..., 1].astype(np.int64) + base[..., 0]))
    with pytest.raises(ValueError):
        cd.extrema_rows(batch, mask_t, W, ops=("median",))
    with pytest.raises(ValueError):
        cd.extrema_rows(batch, mask_t[:, :-1], W)


def test_extrema_where_m4_and_side_stream(sz, oracle):
    import torch
    codec, esz, D, chunk_len, nchunks = "xff", 2, 8, 5120, 5
    rng = np.random.default_rng(33)
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    name, mode, lo, hi, _ = sets[0]
    mask, cnt = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
    for W in (64, 1280):
        with ran(only=["dec_fast"], dec_fast=2):           # the filter launch and the extrema launch
            got = cd.extrema_where(batch, list(map(int, lo)), list(map(int, hi)), window_rows=W, ops=OUTS)
        f = cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)))
        two = cd.extrema_rows(batch, f["mask"], W, ops=OUTS)
        want = em.global_windows(x, chunk_len, D, mask, W)
        assert int(want["count"].sum()) == int(cnt.sum()) > 0
        for k, v in want.items():
            assert np.array_equal(to_np(got[k], esz), v) and np.array_equal(to_np(two[k], esz), v), (W, k)
    # M4 on the 5-chunk walk: 2 000-pixel style windows of 128 rows, with and without a mask
    for m_np, m_t in ((None, None), (mask, torch.from_numpy(mask).cuda())):
        with ran(only=["dec_fast"], dec_fast=1):
            m4 = cd.m4(batch, 128, mask=m_t)
        want = em.global_windows(x, chunk_len, D, m_np, 128)
        names = {"t_first": "first_row", "v_first": "first", "t_min": "argmin", "v_min": "min", "t_max": "argmax", "v_max": "max",
                 "t_last": "last_row", "v_last": "last"}
        assert list(m4) == list(names)
        for k, w in names.items():
            assert np.array_equal(to_np(m4[k], esz), want[w]), k
        nw = -(-(x.size // D) // 128)
        assert m4["t_first"].shape == (nw,) and m4["t_min"].shape == (nw, D) and m4["v_last"].shape == (nw, D)
    full = cd.m4(batch, 128)
    flat = x[:x.size // D * D].reshape(-1, D)
    t = full["t_max"].cpu().numpy()
    assert np.array_equal(flat[t[:, 3], 3], to_np(full["v_max"], esz)[:, 3])        # the time stamps index the decoded batch
    # a side stream: the C entry point and the Python wrapper
    side = torch.cuda.Stream()
    want = em.extrema_rows(x, chunk_len, D, mask, 64)
    with ran(only=["dec_fast"], dec_fast=1):
        check_ext(x, batch, codec, esz, D, chunk_len, mask, 64, ("side stream",), want, stream=side)
    mask_t = torch.from_numpy(mask).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):                          # ChunkedCodec launches on the current stream
        with ran(only=["dec_fast"], dec_fast=1):
            got = cd.extrema_rows(batch, mask_t, 64, per_chunk=True, ops=("min", "count"))
    side.synchronize()
    assert np.array_equal(to_np(got["min"], esz), want["min"]) and np.array_equal(got["count"].cpu().numpy(), want["count"])


def test_extrema_rows_headline_shape(sz, oracle):
    """64 chunks of the headline shape (uint16 x 8, FIRE, 10 KB chunks), filter_rows' band mask from the device, W = 64"""
    codec, esz, D, chunk_len, nchunks, W = "xff", 2, 8, 5120, 64, 64
    rng = np.random.default_rng(64)
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    name, mode, lo, hi, _ = sets[0]
    f = cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)))
    mask = f["mask"].cpu().numpy()
    with ran(only=["dec_fast"], dec_fast=1):
        want = check_ext(x, batch, codec, esz, D, chunk_len, mask, W, ("headline",))
    assert np.array_equal(want["count"].sum(axis=1), f["counts"].cpu().numpy())
