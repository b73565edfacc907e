"""GPU tests (-m gpu) of histogram rows (sprintz_mi355x_histogram_rows, ChunkedCodec.histogram_rows / histogram_where / quantiles):
per-column value counts of the rows a mask names, fused into the decode, in decode_fast.h and decode_kernel.h.  The expected value is
always tests/histogram_model.py applied to the ORIGINAL input -- decode is lossless and pinned elsewhere.  Every launch's kernel family
is asserted, d_hist lies in a sentinel-filled buffer whose padding must keep the sentinel, and rets[nchunks] must stay untouched.
Every batch ends in a short last chunk of whole rows."""
import zlib

import numpy as np
import pytest

import filter_model as fm
import histogram_model as hm
from dispatch import DECODERS, ran
from harness import DTYPES
from fixtures import no_fast, sz  # noqa: F401  (fixtures)
from rowdata import (HS, PARITY_FAST, bound_sets, gen_data, lowdim, make_batch, masked_parity_cases as parity_cases, parity_masks, rows_for,
                     short_batch)
from rowop_runners import check_hist

pytestmark = pytest.mark.gpu

CAP = 16384


def bins_for(D):
    """the most bins (a power of two, at most 256) whose D columns fit a call's counters"""
    nb = 256
    while D * nb > CAP:
        nb //= 2
    return nb


def binnings(rng, x, esz, D):
    """[(name, shift, nbins, lo)]: the bins that cover the range (full resolution at 8 bits, (8, 256, 0) at 16, coarser for wide streams);
    a number of bins that is no power of two; a random lo with wrap-around under fewer bins than the range, so that values fall outside
    and must be dropped; bins of one value around each column's median; one bin"""
    W = 8 * esz
    top = 1 << W
    nb = bins_for(D)
    cover = W - (nb.bit_length() - 1)
    med = np.median(x[:x.size // D * D].reshape(-1, D).astype(np.int64), axis=0).astype(np.int64)
    return [("cover", cover, nb, None), ("no power of two", cover, nb * 3 // 4 + 1, None),
            ("random lo", cover, nb // 2 + 3, rng.integers(1, top, D)), ("around the median", 0, nb, np.mod(med - nb // 3, top)),
            ("one bin", W - 1, 1, rng.integers(1, top, D))]


@pytest.mark.parametrize("codec,esz,D,shape,data", parity_cases())
def test_histogram_rows_parity(sz, oracle, no_fast, codec, esz, D, shape, data):
    """both layouts of the low-dimension shapes x both families: every mask (none, and select's eleven) with the binnings and H walking
    along, and every binning x every H with the masks walking along -- d_hist equals the model"""
    rng = np.random.default_rng(zlib.crc32(f"histogram{codec}{esz}{D}{shape}{data}".encode()))
    R = rows_for(shape, D)
    chunk_len = R * D
    x = gen_data(data, rng, short_batch(5, chunk_len, D), esz, D)
    masks = [("no mask", None)] + parity_masks(rng, x, chunk_len, esz, D)
    bins = binnings(rng, x, esz, D)
    combos = [(mi, mi % len(bins), HS[mi % 4]) for mi in range(len(masks))]
    combos += [((3 * bi + hi) % len(masks), bi, H) for bi in range(len(bins)) for hi, H in enumerate(HS)]
    combos = sorted(set(combos))
    want = {}
    for mi, bi, H in combos:
        _, shift, nbins, lo = bins[bi]
        want[(mi, bi, H)] = hm.histogram_rows(x, chunk_len, D, masks[mi][1], lo, shift, nbins, H)
    for general in ((False, True) if lowdim(esz, D) else (False,)):
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, general)
        first = "dec_fast" if (esz, D, general) in PARITY_FAST else "dec_generic"
        for fam, family in ((0, first), (1, "dec_generic")):
            if fam == 1 and first == "dec_generic":
                continue                                   # (the same kernel again)
            no_fast(fam)
            for mi, bi, H in combos:
                bname, shift, nbins, lo = bins[bi]
                with ran(only=[family], **{family: 1}):
                    check_hist(x, batch, codec, esz, D, chunk_len, masks[mi][1], lo, shift, nbins, H,
                               (codec, esz, D, shape, data, general, family, masks[mi][0], bname, H), want[(mi, bi, H)], general=general)
    # what the model says of the shapes themselves: the covering bins count every sample of every selected row, and no mask is every bit
    nrows = x.size // D
    cover = hm.histogram_rows(x, chunk_len, D, None, None, bins[0][1], bins[0][2], 0)
    assert np.all(cover.sum(axis=2) == nrows)
    assert np.array_equal(cover, hm.histogram_rows(x, chunk_len, D, masks[-1][1], None, bins[0][1], bins[0][2], 0)) and masks[-1][0] == "every bit"
    assert not hm.histogram_rows(x, chunk_len, D, masks[4][1], None, bins[0][1], bins[0][2], 0).any() and masks[4][0] == "no row"
    dropped = hm.histogram_rows(x, chunk_len, D, None, bins[2][3], bins[2][1], bins[2][2], 0)
    if data == "uniform":
        assert np.all(dropped.sum(axis=2) < nrows) and dropped.any()         # values outside the bins were dropped


FAST_SHAPES = [
    # (codec, esz, D, chunk_len, nbins, family without NO_FAST): decode_fast.h's lane mappings -- 4 .. 64 lanes a chunk, 1 / 2 columns a
    # lane, full and partly filled groups -- with tables that fit behind their carves, and two that do not (the generic kernel's)
    ("xff", 2, 8, 5120, 256, "dec_fast"), ("delta", 2, 8, 8 * 648, 1000, "dec_fast"), ("delta", 2, 5, 5 * 1000, 256, "dec_fast"),
    ("xff", 1, 8, 8 * 1024, 256, "dec_fast"), ("delta", 1, 24, 24 * 200, 256, "dec_fast"), ("xff", 2, 24, 24 * 200, 256, "dec_fast"),
    ("xff", 1, 64, 64 * 160, 200, "dec_fast"), ("delta", 1, 80, 10240, 100, "dec_fast"), ("xff", 2, 80, 80 * 128, 16, "dec_fast"),
    ("delta", 2, 128, 128 * 80, 14, "dec_fast"), ("delta", 2, 128, 128 * 80, 15, "dec_generic"), ("xff", 1, 200, 200 * 104, 64, "dec_generic"),
]


@pytest.mark.parametrize("codec,esz,D,chunk_len,nbins,first", FAST_SHAPES)
def test_histogram_rows_fast_mappings(sz, oracle, no_fast, codec, esz, D, chunk_len, nbins, first):
    """the parity matrix's chunks are too short for most of decode_fast.h's mappings: each of them, on chunks it takes, without a mask
    and under select's eleven, at H = 0 and H = 3; the generic kernel on the same batch"""
    rng = np.random.default_rng(zlib.crc32(f"fast{codec}{esz}{D}".encode()))
    W = 8 * esz
    x = gen_data("walk", rng, short_batch(4, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    masks = [("no mask", None)] + parity_masks(rng, x, chunk_len, esz, D)
    shift = max(W - (nbins - 1).bit_length(), 0)
    for i, (name, mask) in enumerate(masks):
        H = (0, 3)[i % 2]
        want = None
        for fam, family in ((0, first), (1, "dec_generic")):
            if fam == 1 and first == "dec_generic":
                continue
            no_fast(fam)
            with ran(only=[family], **{family: 1}):
                want = check_hist(x, batch, codec, esz, D, chunk_len, mask, None, shift, nbins, H, (codec, esz, D, family, name, H), want)


@pytest.mark.parametrize("codec,esz,D,R,nchunks,fam,family,lanes", [
    ("xff", 2, 8, 48, 100, 0, "dec_fast", 8),         # decode_fast.h: 8 lanes a chunk
    ("delta", 1, 8, 48, 100, 1, "dec_generic", 8),    # decode_kernel.h under NO_FAST: choose_mapping(8) is 8 lanes x 1 column
    ("delta", 1, 3, 64, 200, 0, "dec_generic", 4),    # decode_kernel.h, low-dimension layout: 4 lanes a chunk
])
def test_histogram_rows_merges_across_workgroups(sz, oracle, no_fast, codec, esz, D, R, nchunks, fam, family, lanes):
    """H = 0 on a launch of several workgroups: every workgroup's table is added to the one histogram.  geom.h: a workgroup is
    kThreads = 256 lanes, a chunk takes `lanes` of them (one chunk a lane group), so a workgroup decodes 256 / lanes chunks."""
    no_fast(fam)
    wg_chunks = 256 // lanes
    workgroups = -(-nchunks // wg_chunks)
    assert workgroups >= 3 and workgroups == {8: 4, 4: 4}[lanes]
    chunk_len = R * D
    rng = np.random.default_rng(R + D)
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    MB = -(-R // 8)
    mask = np.packbits(rng.random((nchunks, MB * 8)) < 0.5, axis=1, bitorder="little")
    W = 8 * esz
    sel = hm.selected(mask, x.size, chunk_len, D)
    for m, nsel in ((None, x.size // D), (mask, int(sel.sum()))):
        for shift, nbins, lo in ((W - 8, 256, None), (W - 8, 100, rng.integers(1, 1 << W, D))):
            with ran(only=[family], **{family: 1}):
                want = check_hist(x, batch, codec, esz, D, chunk_len, m, lo, shift, nbins, 0, (codec, D, family, m is None, nbins))
            assert want.shape[0] == 1
            rows = hm.selected_values(x, chunk_len, D, m).astype(np.int64)
            lo_v = np.zeros(D, np.int64) if lo is None else lo
            inrange = ((np.mod(rows - lo_v[None, :], 1 << W) >> shift) < nbins).sum(axis=0)
            assert np.array_equal(want[0].sum(axis=1), inrange)              # each column's total: its in-range selected samples
            if lo is None:
                assert np.all(inrange == nsel)
    # a histogram per workgroup's worth of chunks, and one that straddles the workgroups
    for H in (wg_chunks, wg_chunks + 1):
        with ran(only=[family], **{family: 1}):
            check_hist(x, batch, codec, esz, D, chunk_len, mask, None, W - 8, 256, H, (codec, D, family, "H", H))


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz,D", [(2, 8), (1, 16), (1, 3)])
def test_histogram_rows_long_runs(sz, oracle, no_fast, codec, esz, D):
    """constant data, data that is flat for whole chunks behind 40 rows of a walk, and sparse data: runs of hundreds of blocks -- the delta
    shortcut (one add a column of the run's selected rows) against the row loops, FIRE's block-by-block replay -- without a mask and under
    masks whose bytes are partly set inside the runs"""
    R = 2048
    chunk_len = D * R
    W = 8 * esz
    top = (1 << W) - 1
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
    sparse = gen_data("sparse", rng, rows * D, esz, D)
    MB = R // 8
    kinds = {"no mask": None, "3 of 8": np.full((nchunks, MB), 0b00100101, np.uint8), "one stretch": np.zeros((nchunks, MB), np.uint8),
             "p=1/2": np.packbits(rng.random((nchunks, R)) < 0.5, axis=1, bitorder="little"), "no row": np.zeros((nchunks, MB), np.uint8)}
    kinds["one stretch"][:, 40] = 0xF0                      # rows 324 .. 383: starts and ends inside mask bytes
    kinds["one stretch"][:, 41:47] = 0xFF
    kinds["one stretch"][:, 47] = 0x0F
    first = "dec_generic" if lowdim(esz, D) else "dec_fast"
    for label, x in (("constant", const), ("flat chunks", flat), ("sparse", sparse)):
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        for i, (name, mask) in enumerate(kinds.items()):
            H = (0, 1, 2)[i % 3]
            want = hm.histogram_rows(x, chunk_len, D, mask, None, W - 8, 256, H)
            for fam, family in ((0, first), (1, "dec_generic")):
                no_fast(fam)
                with ran(only=[family], **{family: 1}):
                    check_hist(x, batch, codec, esz, D, chunk_len, mask, None, W - 8, 256, H, (codec, esz, D, label, name, H, family), want)
            if label == "constant" and name == "3 of 8":         # 3 rows of every whole 8, and rows 0 and 2 of the last chunk's last 4
                last = rows - (nchunks - 1) * R
                picked = (nchunks - 1) * 3 * (R // 8) + 3 * (last // 8) + bin(0b00100101 & ((1 << (last % 8)) - 1)).count("1")
                assert int(want[:, 0, int(const[0]) >> (W - 8)].sum()) == picked and int(want.sum()) == picked * D
            if name == "one stretch":
                assert int(want[:, 0].sum()) == 56 * nchunks


@pytest.mark.parametrize("codec,esz,D,chunk_len,family", [
    ("xff", 2, 8, 8 * 650, "dec_fast"),           # R = 650: 2 rows in the last mask byte, MB = 82 is no multiple of 4, a verbatim tail of 10 rows
    ("delta", 1, 16, 16 * 203, "dec_fast"),       # R = 203, MB = 26
    ("delta", 2, 3, 3 * 333, "dec_generic"),      # (chunks of 1 998 bytes: no whole 16-byte pieces)
    ("xff", 1, 2, 2 * 1001, "dec_generic"),
])
def test_histogram_rows_mask_edges(sz, oracle, no_fast, codec, esz, D, chunk_len, family):
    """every bit set -- on the short chunk's missing rows and on rows >= R in the last byte too -- counts the existing rows alone, as no
    mask does; and the mask at an odd address with a short last dword (select's read-ahead window, byte by byte)"""
    rng = np.random.default_rng(chunk_len)
    R, MB = fm.geometry(chunk_len, D)
    assert R % 8 and MB % 4
    nchunks = 5
    W = 8 * esz
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    ones = np.full((nchunks, MB), 0xFF, np.uint8)
    half = np.packbits(rng.random((nchunks, MB * 8)) < 0.5, axis=1, bitorder="little")
    for fam, fml in ((0, family), (1, "dec_generic")):
        no_fast(fam)
        for H in (0, 2):
            want = hm.histogram_rows(x, chunk_len, D, None, None, W - 8, 256, H)
            assert int(want.sum()) == x.size
            for shift in (0, 1, 3):
                with ran(only=[fml], **{fml: 2}):
                    check_hist(x, batch, codec, esz, D, chunk_len, ones, None, W - 8, 256, H, (codec, D, fml, H, shift, "every bit"), want, mask_shift=shift)
                    check_hist(x, batch, codec, esz, D, chunk_len, half, None, W - 8, 256, H, (codec, D, fml, H, shift, "p=1/2"), mask_shift=shift)


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [
    ("xff", 2, 8, 5120, 0),       # decode_fast
    ("delta", 1, 80, 10240, 0),   # decode_fast, two columns a lane
    ("xff", 2, 8, 5120, 1),       # decode_kernel (NO_FAST)
    ("delta", 1, 1, 1024, 0),     # decode_kernel, low-dimension layout
])
def test_histogram_rows_damaged_chunk(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    import torch
    no_fast(fam)
    rng = np.random.default_rng(5)
    nchunks, H = 9, 2                                       # five histograms; the damaged chunk 4 lies in histogram 2
    W = 8 * esz
    nbins = min(bins_for(D), 64)
    shift = W - (nbins.bit_length() - 1)
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    bad = 4
    off = int(batch.offsets[bad].item())
    hdr = batch.data[off + 6:off + 8].clone()
    R, MB = fm.geometry(chunk_len, D)
    mask = np.packbits(rng.random((nchunks, MB * 8)) < 0.4, axis=1, bitorder="little")
    mask_t = torch.from_numpy(mask).cuda()
    batch.data[off + 6] = hdr[0] ^ 0x5                  # the header's ndims field
    for m in (mask, None):
        want = check_hist(x, batch, codec, esz, D, chunk_len, m, None, shift, nbins, H, (codec, D, fam, m is None), skip_group=bad // H, bad_chunk=bad)
        assert want.shape[0] == 5
    with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):
        cd.histogram_rows(batch, mask_t, nbins=nbins, chunks_per_hist=H, check=True)
    cd.histogram_rows(batch, mask_t, nbins=nbins, chunks_per_hist=H, check=False)      # no error without the check
    batch.data[off + 6] = hdr[0]
    got = cd.histogram_rows(batch, mask_t, nbins=nbins, chunks_per_hist=H)             # repaired: no error, and exact
    assert np.array_equal(got.cpu().numpy().astype(np.uint64), hm.histogram_rows(x, chunk_len, D, mask, None, shift, nbins, H))


def test_histogram_rows_and_where_python(sz, oracle):
    import torch
    codec, esz, D, chunk_len = "xff", 2, 8, 5120
    rng = np.random.default_rng(21)
    x = gen_data("walk", rng, short_batch(6, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    with ran(only=["dec_fast"], dec_fast=1):
        got = cd.histogram_rows(batch)                      # 256 bins over the range, every row, one histogram
    assert got.dtype == torch.int64 and tuple(got.shape) == (1, D, 256)
    assert np.array_equal(got.cpu().numpy().astype(np.uint64), hm.histogram_rows(x, chunk_len, D, None, None, 8, 256, 0))
    for nbins, want_shift in ((64, 10), (100, 9), (1, 15), (2048, 5)):
        g = cd.histogram_rows(batch, nbins=nbins, chunks_per_hist=4)
        assert tuple(g.shape) == (2, D, nbins) and hm.default_shift(esz, nbins) == want_shift
        assert np.array_equal(g.cpu().numpy().astype(np.uint64), hm.histogram_rows(x, chunk_len, D, None, None, want_shift, nbins, 4)), nbins
    lo = rng.integers(1, 1 << 16, D)
    for lo_arg in (list(map(int, lo)), torch.from_numpy(lo).cuda()):
        g = cd.histogram_rows(batch, nbins=100, lo=lo_arg, shift=3)
        assert np.array_equal(g.cpu().numpy().astype(np.uint64), hm.histogram_rows(x, chunk_len, D, None, lo, 3, 100, 0))
    g = cd.histogram_rows(batch, nbins=16, lo=300, shift=0)
    assert np.array_equal(g.cpu().numpy().astype(np.uint64), hm.histogram_rows(x, chunk_len, D, None, np.full(D, 300), 0, 16, 0))
    sets, _ = bound_sets(x, chunk_len, esz, D)
    for name, mode, flo, fhi, _ in sets[:2]:                # the band (ALL) and the alarm (ANY)
        mask, cnt = fm.filter_rows(x, chunk_len, D, flo, fhi, mode)
        with ran(only=["dec_fast"], dec_fast=2):            # the filter launch and the histogram launch
            got = cd.histogram_where(batch, list(map(int, flo)), list(map(int, fhi)), mode="all" if mode == fm.ALL else "any", nbins=128,
                                     chunks_per_hist=2)
        want = hm.histogram_rows(x, chunk_len, D, mask, None, 9, 128, 2)
        assert np.array_equal(got.cpu().numpy().astype(np.uint64), want), name
        assert int(want[:, 0].sum()) == int(cnt.sum()) > 0
    none = cd.histogram_where(batch, 1, 0)                  # an empty interval: no row
    assert tuple(none.shape) == (1, D, 256) and int(none.sum().item()) == 0
    f = cd.filter_rows(batch, 0, 65535)
    with pytest.raises(ValueError):
        cd.histogram_rows(batch, f["mask"][:, :-1])
    with pytest.raises(sz.SprintzError):
        cd.histogram_rows(batch, nbins=4096)                # 8 x 4096 counters: above the cap
    with pytest.raises(sz.SprintzError):
        cd.histogram_rows(batch, nbins=256, shift=9)        # 256 bins of 512 values are more than the range
    ragged = sz.ChunkedCodec("delta", 1, 80, 1024, device="cuda:0")        # 1 024 elements are no whole rows of 80
    rb = ragged.compress(torch.randint(0, 255, (1024 * 4,), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):
        ragged.histogram_rows(rb, nbins=16)
    with ran(never=DECODERS), pytest.raises(ValueError):    # refused before the filter launches
        ragged.histogram_where(rb, 0, 100, nbins=16)


Q = [0, 0.01, 0.5, 0.99, 1]


@pytest.mark.parametrize("codec,esz,D,chunk_len,data", [
    ("xff", 2, 8, 5120, "walk"), ("delta", 2, 3, 3 * 400, "uniform"), ("delta", 1, 16, 16 * 256, "walk"), ("xff", 1, 4, 4096, "uniform"),
    ("delta", 2, 8, 5120, "constant"),
])
def test_quantiles_python(sz, oracle, codec, esz, D, chunk_len, data):
    """exact quantiles against the sort definition, with and without a mask; 16 bits: a coarse pass and as many refinement passes as a
    column's quantiles have distinct coarse bins"""
    import torch
    rng = np.random.default_rng(D + esz)
    nchunks = 7
    x = gen_data(data, rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    R, MB = fm.geometry(chunk_len, D)
    mask = np.packbits(rng.random((nchunks, MB * 8)) < 0.25, axis=1, bitorder="little")
    for m in (None, mask):
        got = cd.quantiles(batch, Q, mask=None if m is None else torch.from_numpy(m).cuda())
        want = hm.quantiles(x, chunk_len, D, Q, m)
        assert got.dtype == cd.dtype and tuple(got.shape) == (len(Q), D)
        assert np.array_equal(got.cpu().view(torch.int8 if esz == 1 else torch.int16).numpy().view(DTYPES[esz]), want), (codec, esz, D, m is None)
    one = cd.quantiles(batch, 0.5)
    assert np.array_equal(one.cpu().view(torch.int8 if esz == 1 else torch.int16).numpy().view(DTYPES[esz]), hm.quantiles(x, chunk_len, D, [0.5]))
    with pytest.raises(ValueError):
        cd.quantiles(batch, Q, mask=torch.zeros((nchunks, MB), dtype=torch.uint8, device="cuda:0"))      # n = 0
    with pytest.raises(ValueError):
        cd.quantiles(batch, [0.5, 1.5])


def test_quantiles_split_by_lo(sz, oracle):
    """uint8 x 80 columns at full resolution is above a call's counters: two calls of 128 bins, lo = 0 and lo = 128, side by side"""
    import torch
    codec, esz, D, chunk_len, nchunks = "delta", 1, 80, 10240, 5
    rng = np.random.default_rng(80)
    x = gen_data("uniform", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    with ran(only=["dec_generic"], dec_generic=2):          # (44 KB of carves + 40 KB of table are above decode_fast.h's LDS budget)
        got = cd.quantiles(batch, Q)
    assert np.array_equal(got.cpu().numpy(), hm.quantiles(x, chunk_len, D, Q))
    with pytest.raises(sz.SprintzError):
        cd.histogram_rows(batch, nbins=256)
    parts = [cd.histogram_rows(batch, nbins=128, lo=lo, shift=0)[0].cpu().numpy() for lo in (0, 128)]
    assert np.array_equal(np.concatenate(parts, axis=1).astype(np.uint64), hm.histogram_rows(x, chunk_len, D, None, None, 0, 256, 0)[0])


def test_histogram_rows_headline_shape(sz, oracle):
    """the headline shape scaled down: uint16 x 8, FIRE, 10 KB chunks, 2 048 chunks (64 workgroups of decode_fast.h), H = 0, 256 bins"""
    import torch
    codec, esz, D, chunk_len, nchunks = "xff", 2, 8, 5120, 2048
    rng = np.random.default_rng(2048)
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    want = hm.histogram_rows(x, chunk_len, D, None, None, 8, 256, 0)
    with ran(only=["dec_fast"], dec_fast=1):
        check_hist(x, batch, codec, esz, D, chunk_len, None, None, 8, 256, 0, ("headline",), want)
    assert int(want.sum()) == x.size
    with ran(only=["dec_fast"], dec_fast=1):
        got = cd.histogram_rows(batch)
    assert np.array_equal(got.cpu().numpy().astype(np.uint64), want)
