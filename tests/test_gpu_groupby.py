"""GPU tests (-m gpu) of group-by rows (sprintz_mi355x_groupby_rows, ChunkedCodec.groupby_rows / groupby_where): per bin of one key
column's value, the count and the per-column sums of the rows a mask names, fused into the decode, in decode_fast.h and decode_kernel.h.
The expected value is always tests/groupby_model.py applied to the ORIGINAL input -- decode is lossless and pinned elsewhere.  Every
launch's kernel family is asserted, d_count and d_sum lie in sentinel-filled buffers whose padding must keep the sentinel, and
rets[nchunks] must stay untouched.  Every batch ends in a short last chunk of whole rows."""
import zlib

import numpy as np
import pytest

import filter_model as fm
import groupby_model as gm
from dispatch import ran
from harness import DTYPES
from fixtures import no_fast, sz  # noqa: F401  (fixtures)
from rowdata import (HS, PARITY_FAST, bound_sets, gen_data, lowdim, make_batch, masked_parity_cases as parity_cases, parity_masks, rows_for,
                     short_batch)
from rowop_runners import check_gby

pytestmark = pytest.mark.gpu

CAP = 16384


def bins_for(D):
    """the most bins (a power of two, at most 256) whose sums and counts, nbins x (D + 1), fit a call's table"""
    nb = 256
    while (D + 1) * nb > CAP:
        nb //= 2
    return nb


def keys_for(D):
    """the key columns that exercise the hand-over whatever the kernel's lane mapping (1, 2, 4 or 8 columns a lane): column 0 and the
    last one -- for D in {3, 5, 33, 300} the last genuine column of a lane whose other columns do not exist --, columns 1 and 5 (not
    slot 0 of their lane wherever a lane has more than one), and D // 2 and D - 2 (lanes other than lane 0 from 2 columns on)"""
    return sorted(k for k in {0, 1, 5, D // 2, D - 2, D - 1} if 0 <= k < D)


def binnings(rng, x, esz, D, key):
    """[(name, shift, nbins, key_lo)]: the bins that cover the range; a number of bins that is no power of two; a random key_lo with
    wrap-around under fewer bins than the range, so that rows fall outside and must be dropped; bins of one value around the key
    column's median; one bin"""
    W = 8 * esz
    top = 1 << W
    nb = bins_for(D)
    cover = W - (nb.bit_length() - 1)
    med = int(np.median(x[:x.size // D * D].reshape(-1, D)[:, key].astype(np.int64)))
    return [("cover", cover, nb, 0), ("no power of two", cover, nb * 3 // 4 + 1, 0), ("random key_lo", cover, nb // 2 + 3, int(rng.integers(1, top))),
            ("around the median", 0, nb, (med - nb // 3) % top), ("one bin", W - 1, 1, int(rng.integers(1, top)))]


@pytest.mark.parametrize("codec,esz,D,shape,data", parity_cases())
def test_groupby_rows_parity(sz, oracle, no_fast, codec, esz, D, shape, data):
    """both layouts of the low-dimension shapes x both families x every key column of keys_for: every mask (none, and select's eleven)
    with the binnings and H walking along, and every binning x every H with the masks walking along -- d_count and d_sum equal the model"""
    rng = np.random.default_rng(zlib.crc32(f"groupby{codec}{esz}{D}{shape}{data}".encode()))
    R = rows_for(shape, D)
    chunk_len = R * D
    x = gen_data(data, rng, short_batch(5, chunk_len, D), esz, D)
    masks = [("no mask", None)] + parity_masks(rng, x, chunk_len, esz, D)
    assert len(masks) == 12
    keys = keys_for(D)
    bins = {key: binnings(rng, x, esz, D, key) for key in keys}
    nb = len(bins[keys[0]])
    combos = [(mi, mi % nb, HS[mi % 4]) for mi in range(len(masks))]
    combos += [((3 * bi + hi) % len(masks), bi, H) for bi in range(nb) for hi, H in enumerate(HS)]
    combos = sorted(set(combos))
    want = {}
    for key in keys:
        for mi, bi, H in combos:
            _, shift, nbins, key_lo = bins[key][bi]
            want[(key, mi, bi, H)] = gm.groupby_rows(x, chunk_len, D, key, masks[mi][1], key_lo, shift, nbins, H)
    for general in ((False, True) if lowdim(esz, D) else (False,)):
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, general)
        first = "dec_fast" if (esz, D, general) in PARITY_FAST else "dec_generic"
        for fam, family in ((0, first), (1, "dec_generic")):
            if fam == 1 and first == "dec_generic":
                continue                                   # (the same kernel again)
            no_fast(fam)
            for key in keys:
                for mi, bi, H in combos:
                    bname, shift, nbins, key_lo = bins[key][bi]
                    with ran(only=[family], **{family: 1}):
                        check_gby(x, batch, codec, esz, D, chunk_len, key, masks[mi][1], key_lo, shift, nbins, H,
                                  (codec, esz, D, shape, data, general, family, key, masks[mi][0], bname, H), want[(key, mi, bi, H)], general=general)
    # what the model says of the shapes themselves: the covering bins hold every selected row, no mask is every bit, and rows were dropped
    nrows = x.size // D
    rows = x[:nrows * D].reshape(-1, D).astype(np.uint64)
    key = keys[-1]
    cnt, tot = gm.groupby_rows(x, chunk_len, D, key, None, 0, bins[key][0][1], bins[key][0][2], 0)
    assert int(cnt.sum()) == nrows and np.array_equal(tot.sum(axis=(0, 1)), rows.sum(axis=0))
    every = gm.groupby_rows(x, chunk_len, D, key, masks[-1][1], 0, bins[key][0][1], bins[key][0][2], 0)
    assert np.array_equal(cnt, every[0]) and np.array_equal(tot, every[1]) and masks[-1][0] == "every bit"
    assert not gm.groupby_rows(x, chunk_len, D, key, masks[4][1], 0, bins[key][0][1], bins[key][0][2], 0)[0].any() and masks[4][0] == "no row"
    if data == "uniform":
        dropped = gm.groupby_rows(x, chunk_len, D, key, None, bins[key][2][3], bins[key][2][1], bins[key][2][2], 0)[0]
        assert 0 < int(dropped.sum()) < nrows


FAST_SHAPES = [
    # (codec, esz, D, chunk_len, nbins, family without NO_FAST): decode_fast.h's lane mappings -- 4 .. 64 lanes a chunk, 1 / 2 columns a
    # lane, full and partly filled groups -- with tables that fit behind their carves, and two that do not (the generic kernel's)
    ("xff", 2, 8, 5120, 256, "dec_fast"), ("delta", 2, 8, 8 * 648, 1000, "dec_fast"), ("delta", 2, 5, 5 * 1000, 256, "dec_fast"),
    ("xff", 1, 8, 8 * 1024, 256, "dec_fast"), ("delta", 1, 24, 24 * 200, 256, "dec_fast"), ("xff", 2, 24, 24 * 200, 256, "dec_fast"),
    ("xff", 1, 64, 64 * 160, 200, "dec_fast"), ("delta", 1, 80, 10240, 100, "dec_fast"), ("xff", 2, 80, 80 * 128, 16, "dec_fast"),
    ("delta", 2, 128, 128 * 80, 14, "dec_fast"), ("delta", 2, 128, 128 * 80, 15, "dec_generic"), ("xff", 1, 200, 200 * 104, 64, "dec_generic"),
]


@pytest.mark.parametrize("codec,esz,D,chunk_len,nbins,first", FAST_SHAPES)
def test_groupby_rows_fast_mappings(sz, oracle, no_fast, codec, esz, D, chunk_len, nbins, first):
    """the parity matrix's chunks are too short for most of decode_fast.h's mappings: each of them, on chunks it takes, without a mask
    and under select's eleven, at H = 0 and H = 3, the key columns walking along; the generic kernel on the same batch"""
    rng = np.random.default_rng(zlib.crc32(f"fast{codec}{esz}{D}".encode()))
    W = 8 * esz
    x = gen_data("walk", rng, short_batch(4, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    masks = [("no mask", None)] + parity_masks(rng, x, chunk_len, esz, D)
    keys = keys_for(D)
    shift = max(W - (nbins - 1).bit_length(), 0)
    for i, (name, mask) in enumerate(masks):
        H = (0, 3)[i % 2]
        for key in (keys[i % len(keys)], keys[(i + 3) % len(keys)]):
            want = None
            for fam, family in ((0, first), (1, "dec_generic")):
                if fam == 1 and first == "dec_generic":
                    continue
                no_fast(fam)
                with ran(only=[family], **{family: 1}):
                    want = check_gby(x, batch, codec, esz, D, chunk_len, key, mask, 0, shift, nbins, H, (codec, esz, D, family, key, name, H), want)


@pytest.mark.parametrize("codec,esz,D,R,nchunks,fam,family,lanes", [
    ("xff", 2, 8, 48, 100, 0, "dec_fast", 8),         # decode_fast.h: 8 lanes a chunk
    ("delta", 1, 8, 48, 100, 1, "dec_generic", 8),    # decode_kernel.h under NO_FAST: choose_mapping(8) is 8 lanes x 1 column
    ("delta", 1, 3, 64, 200, 0, "dec_generic", 4),    # decode_kernel.h, low-dimension layout: 4 lanes a chunk
])
def test_groupby_rows_merges_across_workgroups(sz, oracle, no_fast, codec, esz, D, R, nchunks, fam, family, lanes):
    """H = 0 on a launch of several workgroups: every workgroup's table is added to the one table; fewer chunks than a workgroup holds
    and a single chunk; a table per workgroup's worth of chunks, and one that straddles the workgroups"""
    no_fast(fam)
    wg_chunks = 256 // lanes
    assert -(-nchunks // wg_chunks) == 4
    chunk_len = R * D
    rng = np.random.default_rng(R + D)
    W = 8 * esz
    MB = -(-R // 8)
    for n in (nchunks, wg_chunks // 2 + 1, 1):
        x = gen_data("walk", rng, short_batch(n, chunk_len, D), esz, D)
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        mask = np.packbits(rng.random((n, MB * 8)) < 0.5, axis=1, bitorder="little")
        for m in (None, mask):
            for key, shift, nbins, key_lo in ((0, W - 8, 256, 0), (D - 1, W - 8, 100, int(rng.integers(1, 1 << W)))):
                with ran(only=[family], **{family: 1}):
                    want = check_gby(x, batch, codec, esz, D, chunk_len, key, m, key_lo, shift, nbins, 0, (codec, D, family, n, m is None, nbins))
                assert want[0].shape[0] == 1
                if m is None and key_lo == 0:
                    assert int(want[0].sum()) == x.size // D
        for H in ((wg_chunks, wg_chunks + 1) if n == nchunks else (1,)):
            with ran(only=[family], **{family: 1}):
                check_gby(x, batch, codec, esz, D, chunk_len, 1, mask, 0, W - 8, 256, H, (codec, D, family, n, "H", H))


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz,D", [(2, 8), (1, 16), (1, 3)])
def test_groupby_rows_long_runs(sz, oracle, no_fast, codec, esz, D):
    """runs of hundreds of blocks -- the delta shortcut (each column adds its value times the run's selected rows) against the row loops,
    FIRE's block-by-block replay -- without a mask and under masks whose bits cut the runs in the middle: constant data, data that is flat
    for whole chunks behind 40 rows of a walk, sparse data, the key column alone constant, and the key column alone varying"""
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
    key = D - 2
    walk = gen_data("walk", rng, rows * D, esz, D).reshape(rows, D)
    key_const = walk.copy()
    key_const[:, key] = 0x77
    key_varies = np.full((rows, D), 0x33, DTYPES[esz])
    key_varies[:, key] = walk[:, key]
    MB = R // 8
    kinds = {"no mask": None, "3 of 8": np.full((nchunks, MB), 0b00100101, np.uint8), "one stretch": np.zeros((nchunks, MB), np.uint8),
             "p=1/2": np.packbits(rng.random((nchunks, R)) < 0.5, axis=1, bitorder="little"), "no row": np.zeros((nchunks, MB), np.uint8)}
    kinds["one stretch"][:, 40] = 0xF0                      # rows 324 .. 383: starts and ends inside mask bytes
    kinds["one stretch"][:, 41:47] = 0xFF
    kinds["one stretch"][:, 47] = 0x0F
    first = "dec_generic" if lowdim(esz, D) else "dec_fast"
    for label, x in (("constant", const), ("flat chunks", flat), ("sparse", sparse), ("key constant", key_const.ravel()), ("key varies", key_varies.ravel())):
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        for i, (name, mask) in enumerate(kinds.items()):
            H = (0, 1, 2)[i % 3]
            k = (key, 0)[i % 2]
            want = gm.groupby_rows(x, chunk_len, D, k, mask, 0, W - 8, 256, H)
            for fam, family in ((0, first), (1, "dec_generic")):
                no_fast(fam)
                with ran(only=[family], **{family: 1}):
                    check_gby(x, batch, codec, esz, D, chunk_len, k, mask, 0, W - 8, 256, H, (codec, esz, D, label, name, H, family), want)
            if label == "constant" and name == "3 of 8":         # 3 rows of every whole 8, and rows 0 and 2 of the last chunk's last 4
                last = rows - (nchunks - 1) * R
                picked = (nchunks - 1) * 3 * (R // 8) + 3 * (last // 8) + bin(0b00100101 & ((1 << (last % 8)) - 1)).count("1")
                b = int(const[0]) >> (W - 8)
                assert int(want[0][:, b].sum()) == picked == int(want[0].sum()) and np.all(want[1][:, b].sum(axis=0) == picked * int(const[0]))
            if name == "one stretch":
                assert int(want[0].sum()) == 56 * nchunks


@pytest.mark.parametrize("codec,esz,D,chunk_len,family", [
    ("xff", 2, 8, 8 * 650, "dec_fast"),           # R = 650: 2 rows in the last mask byte, MB = 82 is no multiple of 4, a verbatim tail of 10 rows
    ("delta", 1, 16, 16 * 203, "dec_fast"),       # R = 203, MB = 26
    ("delta", 2, 3, 3 * 333, "dec_generic"),      # (chunks of 1 998 bytes: no whole 16-byte pieces)
    ("xff", 1, 2, 2 * 1001, "dec_generic"),
])
def test_groupby_rows_mask_edges(sz, oracle, no_fast, codec, esz, D, chunk_len, family):
    """every bit set -- on the short chunk's missing rows and on rows >= R in the last byte too -- selects the existing rows alone, as no
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
    key = D - 1
    for fam, fml in ((0, family), (1, "dec_generic")):
        no_fast(fam)
        for H in (0, 2):
            want = gm.groupby_rows(x, chunk_len, D, key, None, 0, W - 8, 256, H)
            assert int(want[0].sum()) == x.size // D
            for shift in (0, 1, 3):
                with ran(only=[fml], **{fml: 2}):
                    check_gby(x, batch, codec, esz, D, chunk_len, key, ones, 0, W - 8, 256, H, (codec, D, fml, H, shift, "every bit"), want, mask_shift=shift)
                    check_gby(x, batch, codec, esz, D, chunk_len, key, half, 0, W - 8, 256, H, (codec, D, fml, H, shift, "p=1/2"), mask_shift=shift)


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam,family", [
    ("xff", 2, 8, 5120, 0, "dec_fast"), ("delta", 1, 80, 10240, 0, "dec_fast"), ("delta", 2, 8, 5120, 1, "dec_generic"),
    ("delta", 1, 3, 3 * 512, 0, "dec_generic"),
])
def test_groupby_rows_ops_subsets(sz, oracle, no_fast, codec, esz, D, chunk_len, fam, family):
    """each subset of ops: the output that is not selected may be NULL, and a buffer that is passed for it comes back untouched"""
    no_fast(fam)
    rng = np.random.default_rng(D + chunk_len)
    W = 8 * esz
    nchunks = 6
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    R, MB = fm.geometry(chunk_len, D)
    mask = np.packbits(rng.random((nchunks, MB * 8)) < 0.3, axis=1, bitorder="little")
    nbins = min(bins_for(D), 64)            # (uint8 x 80: a table that still fits behind decode_fast.h's carves)
    shift = W - (nbins.bit_length() - 1)
    for H in (0, 1, 4):                                     # the table; the direct path; tables that cut a workgroup's chunks
        for m in (None, mask):
            want = gm.groupby_rows(x, chunk_len, D, D // 2, m, 0, shift, nbins, H)
            for ops in (1, 2, 3):
                for passed in (False, True):
                    with ran(only=[family], **{family: 1}):
                        check_gby(x, batch, codec, esz, D, chunk_len, D // 2, m, 0, shift, nbins, H, (codec, D, family, H, m is None, ops, passed), want,
                                  ops=ops, pass_unselected=passed)


@pytest.mark.parametrize("fam,family", [(0, "dec_fast"), (1, "dec_generic")])
@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_groupby_rows_exact_near_the_wrap(sz, oracle, no_fast, codec, fam, family):
    """constant 0xFFFF data, uint16 x 8, 32 chunks a workgroup, every row in one bin.  2048 rows a chunk: the planner gives the table
    (65536 rows x 65535 = 0xFFFF0000, the largest 32-bit entry there can be: 65537 rows would be 2^32 - 1), and a workgroup's entry of
    every column reaches it.  2049 rows a chunk: one row too many, every add goes to global memory.  Both are exact
    (tests/test_groupby_cpu.py pins the same two shapes' plans)"""
    no_fast(fam)
    esz, D, nchunks = 2, 8, 34                              # a full workgroup of 32 chunks, and a second one with a short last chunk
    for R in (2048, 2049):
        chunk_len = R * D
        x = np.full(short_batch(nchunks, chunk_len, D), 0xFFFF, np.uint16)
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        nrows = x.size // D
        MB = -(-R // 8)
        for key, key_lo, shift, nbins, b in ((3, 0, 8, 256, 255), (7, 0xFFFF, 0, 1, 0)):
            for mask, sel in ((None, nrows), (np.full((nchunks, MB), 0b10110111, np.uint8), None)):
                want = gm.groupby_rows(x, chunk_len, D, key, mask, key_lo, shift, nbins, 0)
                if sel is not None:
                    assert int(want[0][0, b]) == sel == int(want[0].sum()) and np.all(want[1][0, b] == sel * 0xFFFF)
                    assert 32 * R * 0xFFFF == (0xFFFF0000 if R == 2048 else 0xFFFF0000 + 32 * 0xFFFF) and sel > 32 * R
                with ran(only=[family], **{family: 1}):
                    check_gby(x, batch, codec, esz, D, chunk_len, key, mask, key_lo, shift, nbins, 0, (codec, family, R, key, mask is None), want)
        with ran(only=[family], **{family: 1}):             # a table per workgroup: the first one's entries are the 32 chunks' alone
            want = check_gby(x, batch, codec, esz, D, chunk_len, 0, None, 0, 8, 256, 32, (codec, family, R, "H = 32"))
        assert int(want[1][0, 255, 0]) == 32 * R * 0xFFFF


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [
    ("xff", 2, 8, 5120, 0),       # decode_fast
    ("delta", 1, 80, 10240, 0),   # decode_fast, two columns a lane
    ("xff", 2, 8, 5120, 1),       # decode_kernel (NO_FAST)
    ("delta", 1, 1, 1024, 0),     # decode_kernel, low-dimension layout
])
def test_groupby_rows_damaged_chunk(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    import torch
    no_fast(fam)
    rng = np.random.default_rng(5)
    nchunks, H = 9, 2                                       # five tables; the damaged chunk 4 lies in table 2
    W = 8 * esz
    nbins = min(bins_for(D), 64)
    shift = W - (nbins.bit_length() - 1)
    key = D // 2
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
        want = check_gby(x, batch, codec, esz, D, chunk_len, key, m, 0, shift, nbins, H, (codec, D, fam, m is None), skip_table=bad // H, bad_chunk=bad)
        assert want[0].shape[0] == 5
    with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):
        cd.groupby_rows(batch, key, nbins=nbins, mask=mask_t, chunks_per_table=H, check=True)
    cd.groupby_rows(batch, key, nbins=nbins, mask=mask_t, chunks_per_table=H, check=False)       # no error without the check
    batch.data[off + 6] = hdr[0]
    got = cd.groupby_rows(batch, key, nbins=nbins, mask=mask_t, chunks_per_table=H)              # repaired: no error, and exact
    want = gm.groupby_rows(x, chunk_len, D, key, mask, 0, shift, nbins, H)
    assert np.array_equal(got["count"].cpu().numpy().astype(np.uint64), want[0]) and np.array_equal(got["sum"].cpu().numpy().astype(np.uint64), want[1])


def ulps(a, b):
    """the distance of two float64 arrays in units in the last place (both finite, same sign)"""
    return np.abs(a.view(np.int64) - b.view(np.int64))


def test_groupby_rows_and_where_python(sz, oracle):
    import torch
    codec, esz, D, chunk_len = "xff", 2, 8, 5120
    rng = np.random.default_rng(21)
    x = gen_data("walk", rng, short_batch(6, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    with ran(only=["dec_fast"], dec_fast=1):
        got = cd.groupby_rows(batch, 2)                     # 256 bins over the key's range, every row, one table
    assert set(got) == {"count", "sum", "mean"}
    assert got["count"].dtype == got["sum"].dtype == torch.int64 and got["mean"].dtype == torch.float64
    assert tuple(got["count"].shape) == (1, 256) and tuple(got["sum"].shape) == tuple(got["mean"].shape) == (1, 256, D)
    wc, ws = gm.groupby_rows(x, chunk_len, D, 2, None, 0, 8, 256, 0)
    assert np.array_equal(got["count"].cpu().numpy().astype(np.uint64), wc) and np.array_equal(got["sum"].cpu().numpy().astype(np.uint64), ws)
    # mean: sum / count in float64 -- two correctly rounded conversions and one division are within 3 ulp of the quotient of the
    # integers; 4 allowed -- and NaN exactly where count is 0
    mean = got["mean"].cpu().numpy()
    assert np.array_equal(np.isnan(mean), np.broadcast_to((wc == 0)[..., None], mean.shape)) and (wc == 0).any() and (wc > 0).any()
    ref = gm.mean(wc, ws)
    ok = ~np.isnan(ref)
    assert int(ulps(mean[ok], ref[ok]).max()) <= 4
    for nbins, want_shift in ((64, 10), (100, 9), (1, 15), (1820, 5)):
        g = cd.groupby_rows(batch, D - 1, nbins=nbins, chunks_per_table=4)
        assert tuple(g["count"].shape) == (2, nbins) and gm.default_shift(esz, nbins) == want_shift
        wc, ws = gm.groupby_rows(x, chunk_len, D, D - 1, None, 0, want_shift, nbins, 4)
        assert np.array_equal(g["count"].cpu().numpy().astype(np.uint64), wc) and np.array_equal(g["sum"].cpu().numpy().astype(np.uint64), ws), nbins
    g = cd.groupby_rows(batch, 0, nbins=100, key_lo=40000, shift=3, ops="sum")
    assert set(g) == {"sum"}
    assert np.array_equal(g["sum"].cpu().numpy().astype(np.uint64), gm.groupby_rows(x, chunk_len, D, 0, None, 40000, 3, 100, 0)[1])
    g = cd.groupby_rows(batch, 0, nbins=16, key_lo=300, shift=0, ops=("count",))
    assert set(g) == {"count"}
    assert np.array_equal(g["count"].cpu().numpy().astype(np.uint64), gm.groupby_rows(x, chunk_len, D, 0, None, 300, 0, 16, 0)[0])
    sets, _ = bound_sets(x, chunk_len, esz, D)
    for name, mode, flo, fhi, _ in sets[:2]:                # the band (ALL) and the alarm (ANY)
        mask, cnt = fm.filter_rows(x, chunk_len, D, flo, fhi, mode)
        with ran(only=["dec_fast"], dec_fast=2):            # the filter launch and the group-by launch
            got = cd.groupby_where(batch, list(map(int, flo)), list(map(int, fhi)), mode="all" if mode == fm.ALL else "any", key=3, nbins=128,
                                   chunks_per_table=2)
        wc, ws = gm.groupby_rows(x, chunk_len, D, 3, mask, 0, 9, 128, 2)
        assert np.array_equal(got["count"].cpu().numpy().astype(np.uint64), wc) and np.array_equal(got["sum"].cpu().numpy().astype(np.uint64), ws), name
        assert int(wc.sum()) == int(cnt.sum()) > 0
        m = got["mean"].cpu().numpy()
        assert np.array_equal(np.isnan(m[..., 0]), wc == 0)
    none = cd.groupby_where(batch, 1, 0, key=0)             # an empty interval: no row
    assert int(none["count"].sum().item()) == 0 and int(none["sum"].sum().item()) == 0 and bool(torch.isnan(none["mean"]).all().item())
    f = cd.filter_rows(batch, 0, 65535)
    with pytest.raises(ValueError):
        cd.groupby_rows(batch, 0, mask=f["mask"][:, :-1])
    with pytest.raises(ValueError):
        cd.groupby_rows(batch, D)                           # no such column
    with pytest.raises(ValueError):
        cd.groupby_rows(batch, 0, ops=("count", "max"))
    with pytest.raises(sz.SprintzError):
        cd.groupby_rows(batch, 0, nbins=1821)               # 1821 x 9 entries: above the cap
    with pytest.raises(sz.SprintzError):
        cd.groupby_rows(batch, 0, nbins=256, shift=9)       # 256 bins of 512 values are more than the range
    ragged = sz.ChunkedCodec("delta", 1, 80, 1024, device="cuda:0")        # 1 024 elements are no whole rows of 80
    rb = ragged.compress(torch.randint(0, 255, (1024 * 4,), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):
        ragged.groupby_rows(rb, 0, nbins=16)


def test_groupby_rows_headline_shape(sz, oracle):
    """the headline shape scaled down: uint16 x 8, FIRE, 10 KB chunks, 2 048 chunks (64 workgroups of decode_fast.h), H = 0, 256 bins"""
    codec, esz, D, chunk_len, nchunks = "xff", 2, 8, 5120, 2048
    rng = np.random.default_rng(2048)
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    want = gm.groupby_rows(x, chunk_len, D, 0, None, 0, 8, 256, 0)
    with ran(only=["dec_fast"], dec_fast=1):
        check_gby(x, batch, codec, esz, D, chunk_len, 0, None, 0, 8, 256, 0, ("headline",), want)
    assert int(want[0].sum()) == x.size // D
    with ran(only=["dec_fast"], dec_fast=1):
        got = cd.groupby_rows(batch, 0)
    assert np.array_equal(got["count"].cpu().numpy().astype(np.uint64), want[0]) and np.array_equal(got["sum"].cpu().numpy().astype(np.uint64), want[1])
