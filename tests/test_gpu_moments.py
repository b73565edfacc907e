"""GPU tests (-m gpu) of moments rows (sprintz_mi355x_moments_rows, ChunkedCodec.moments_rows / moments_where / corr): per-window
count, sum, sum of squares and sum of products with one reference column of the rows a mask names, fused into the decode, in
decode_fast.h and decode_kernel.h.  The expected value is always tests/moments_model.py applied to the ORIGINAL input -- decode is
lossless and pinned elsewhere.  Every launch's kernel family is asserted, every output lies in a sentinel-filled buffer whose padding
must keep the sentinel, and rets[nchunks] must stay untouched.  Integer outputs are compared for equality.  Every batch of the parity
tiers ends in a short last chunk of whole rows."""
import zlib
from fractions import Fraction

import numpy as np
import pytest

import filter_model as fm
import moments_model as mm
from dispatch import ran
from harness import DTYPES
from moments_model import U, corr_bound
from fixtures import no_fast, sz  # noqa: F401  (fixtures)
from rowdata import (DATA, FAST_SHAPES, MASKED_NDIMS as NDIMS, MASKED_SHAPES as SHAPES, PARITY_FAST, bound_sets, gen_data, lowdim, make_batch,
                     parity_masks, rows_for, short_batch, windows_for)
from rowop_runners import check_mom

pytestmark = pytest.mark.gpu


def refs_for(D):
    return sorted({0, D - 1, D // 2})


def parity_cases():
    """test_aggregate_rows_parity's matrix: codec x esz x ndims in full; per (codec, esz) the ndims walk the three chunk shapes and the
    four kinds of data"""
    cases = []
    for codec in ("delta", "xff"):
        for esz in (1, 2):
            for j, D in enumerate(NDIMS):
                cases.append((codec, esz, D, SHAPES[j % 3], DATA[(j + (1 if codec == "xff" else 0) + 2 * (esz - 1)) % 4]))
    return cases


@pytest.mark.parametrize("codec,esz,D,shape,data", parity_cases())
def test_moments_rows_parity(sz, oracle, no_fast, codec, esz, D, shape, data):
    """both layouts of the low-dimension shapes x (eleven masks + no mask) x five windows x the reference column in the first lane, the
    last genuine lane and a middle slot x both families: every output equals the model"""
    rng = np.random.default_rng(zlib.crc32(f"moments{codec}{esz}{D}{shape}{data}".encode()))
    R = rows_for(shape, D)
    chunk_len = R * D
    x = gen_data(data, rng, short_batch(5, chunk_len, D), esz, D)
    masks = parity_masks(rng, x, chunk_len, esz, D) + [("none", None)]
    assert len(masks) == 12
    want = {(name, W, ref): mm.moments_rows(x, chunk_len, D, mask, W, ref) for name, mask in masks for W in windows_for(R) for ref in refs_for(D)}
    for general in ((False, True) if lowdim(esz, D) else (False,)):
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, general)
        first = "dec_fast" if (esz, D, general) in PARITY_FAST else "dec_generic"
        for fam, family in ((0, first), (1, "dec_generic")):
            if fam == 1 and first == "dec_generic":
                continue                                   # (the same kernel again)
            no_fast(fam)
            for name, mask in masks:
                for W in windows_for(R):
                    for ref in refs_for(D):
                        with ran(only=[family], **{family: 1}):
                            check_mom(x, batch, codec, esz, D, chunk_len, mask, W, ref, (codec, esz, D, shape, data, general, family, name, W, ref),
                                      want[(name, W, ref)], general=general)
    assert int(want[("no row", 8, 0)]["count"].sum()) == 0
    assert int(want[("every bit", 8, 0)]["count"].sum()) == x.size // D == int(want[("none", 8, 0)]["count"].sum())
    assert int(want[("row 0", 8, 0)]["count"].sum()) == 5


def slot_refs(D):
    """two reference columns that fall in the first and in the last slot of a lane whichever of decode_fast.h's mappings -- 1, 2 or 4
    columns a lane, column = lane * CPL + slot -- the planner picks: a multiple of 4, and a column that is 3 modulo 4"""
    refs = [(D // 2) // 4 * 4, (D - 4) // 4 * 4 + 3]
    assert all(0 <= r < D for r in refs)
    for CPL in (1, 2, 4):
        assert {r % CPL for r in refs} == {0, CPL - 1}, (D, CPL, refs)     # both occurred, under every mapping
    return refs


@pytest.mark.parametrize("codec,esz,D,chunk_len", FAST_SHAPES)
def test_moments_rows_fast_mappings(sz, oracle, no_fast, codec, esz, D, chunk_len):
    """the parity matrix's chunks are too short for most of decode_fast.h's mappings: each of them, on chunks it takes, with the
    reference column in the first and in the last slot of a lane (the second forces products of slots decoded before the
    reference's), under the eleven masks and none, at a window inside the chunk and at one window a chunk; the generic kernel on the
    same batch"""
    rng = np.random.default_rng(zlib.crc32(f"momfast{codec}{esz}{D}".encode()))
    R = chunk_len // D
    refs = slot_refs(D)
    x = gen_data("walk", rng, short_batch(4, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    masks = parity_masks(rng, x, chunk_len, esz, D) + [("none", None)]
    for W in (24, -(-R // 8) * 8):
        for name, mask in masks:
            for ref in refs:
                want = None
                for fam, family in ((0, "dec_fast"), (1, "dec_generic")):
                    no_fast(fam)
                    with ran(only=[family], **{family: 1}):
                        want = check_mom(x, batch, codec, esz, D, chunk_len, mask, W, ref, (codec, esz, D, family, name, W, ref), want)


def carry_data(kind, rng, esz, D, rows):
    top = (1 << (8 * esz)) - 1
    if kind == "constant":                                   # (a) the delta-run shortcut's 64-bit multiplies
        return np.full(rows * D, top, DTYPES[esz])
    if kind == "top16":                                      # (b) no runs: a block's 8 products exceed 2^32 at 16 bits
        return rng.integers(top - 15, top + 1, rows * D).astype(DTYPES[esz])
    # (c) a sawtooth that steps across 0 and the type's maximum: wrapped running values, garbage above bit W in the decoders' registers
    t = (np.arange(rows)[:, None] * (top // 5 + 1) + np.arange(D)[None, :] * 37) % (top + 1)
    t[(np.arange(rows) // 7) % 2 == 1] = (top - t[(np.arange(rows) // 7) % 2 == 1])
    return t.astype(DTYPES[esz]).ravel()


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz,D", [(2, 8), (1, 16)])
@pytest.mark.parametrize("kind", ["constant", "top16", "sawtooth"])
def test_moments_rows_carries(sz, oracle, no_fast, codec, esz, D, kind):
    """the largest products, on both families.  At 16 bits the sums' carries leave 32 bits inside one block and inside every window of
    64 rows, which the model's own sumsq and cross are asserted to show.  At 8 bits they cannot: 2 048 rows of 255^2 stay below 2^32,
    so those cases drive no 64-bit carry within a chunk -- only the 32-bit block sums and the 64-bit adds behind them"""
    R = 2048
    chunk_len = D * R
    nchunks = 3
    rng = np.random.default_rng(esz * 100 + D)
    x = carry_data(kind, rng, esz, D, nchunks * R - 700)
    MB = R // 8
    kinds = {"every row": np.full((nchunks, MB), 0xFF, np.uint8), "3 of 8": np.full((nchunks, MB), 0b00100101, np.uint8),
             "one window": np.zeros((nchunks, MB), np.uint8), "none": None}
    kinds["one window"][:, 5 * 8:6 * 8] = 0xFF
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    ref = D - 1
    for W in (R, 64):
        for name, mask in kinds.items():
            want = mm.moments_rows(x, chunk_len, D, mask, W, ref)
            if kind != "sawtooth" and esz == 2 and name in ("every row", "none"):
                assert int(want["sumsq"].min(initial=1 << 63, where=want["count"][..., None] >= 64)) > 1 << 32
                assert int(want["cross"].max()) > 1 << 32
            for fam, family in ((0, "dec_fast"), (1, "dec_generic")):
                no_fast(fam)
                with ran(only=[family], **{family: 1}):
                    check_mom(x, batch, codec, esz, D, chunk_len, mask, W, ref, (codec, esz, D, kind, name, W, family), want)


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz,D", [(2, 8), (1, 16), (1, 3)])
def test_moments_rows_long_runs(sz, oracle, no_fast, codec, esz, D):
    """test_aggregate_rows_long_runs' two batches -- constant, and flat for whole chunks behind 40 rows of a walk (the run starts inside
    a window): runs of hundreds of blocks that cross many windows -- decode_fast.h's delta shortcut against the row loops -- under a
    mask of 3 rows of every 8, one of a single window, every row, none of them, and without a mask"""
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
             "every row": np.full((nchunks, MB), 0xFF, np.uint8), "no row": np.zeros((nchunks, MB), np.uint8), "none": None}
    kinds["one window"][:, 5 * 8:6 * 8] = 0xFF             # rows 320 .. 383: window 5 of 64 rows
    first = "dec_generic" if lowdim(esz, D) else "dec_fast"
    ref = D // 2
    for label, x in (("constant", const), ("flat chunks", flat)):
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        for name, mask in kinds.items():
            for W in (64, 72, R):
                want = mm.moments_rows(x, chunk_len, D, mask, W, ref)
                for fam, family in ((0, first), (1, "dec_generic")):
                    no_fast(fam)
                    with ran(only=[family], **{family: 1}):
                        check_mom(x, batch, codec, esz, D, chunk_len, mask, W, ref, (codec, esz, D, label, name, W, family), want)
                if name == "one window" and W == 64:
                    assert np.all(want["count"][:2, 5] == 64) and int(want["count"].sum()) == 64 * 3
                if name == "3 of 8" and label == "constant" and R % W == 0:
                    assert np.all(want["sumsq"][0] == np.uint64(int(const[0]) ** 2 * 3 * (W // 8)))


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam,family", [
    ("xff", 2, 8, 5120, 0, "dec_fast"),
    ("delta", 1, 80, 10240, 0, "dec_fast"),
    ("delta", 2, 12, 12 * 400, 0, "dec_fast"),    # (a reduce-only mode: rows need not be whole 16-byte pieces)
    ("delta", 1, 1, 1024, 0, "dec_generic"),
    ("xff", 1, 3, 3000, 0, "dec_generic"),
    ("delta", 2, 300, 9600, 0, "dec_generic"),
    ("xff", 2, 8, 5120, 1, "dec_generic"),
])
def test_moments_rows_each_op_alone(sz, oracle, no_fast, codec, esz, D, chunk_len, fam, family):
    """each op alone, pairs and all four, under two sentinels: an output that is not selected stays untouched -- given, or NULL; a
    reference column that does not exist is accepted where the cross products are not selected"""
    no_fast(fam)
    rng = np.random.default_rng(D + fam)
    x = gen_data("walk", rng, short_batch(6, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    name, mode, lo, hi, _ = sets[0]
    mask, cnt = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
    assert 0 < int(cnt.sum()) < x.size // D
    ref = D // 2
    for W in (64, -(-(chunk_len // D) // 8) * 8):
        want = mm.moments_rows(x, chunk_len, D, mask, W, ref)
        assert np.array_equal(want["count"].sum(axis=1), cnt)
        for ops, byte in ((1, 0x5A), (2, 0xA5), (4, 0x5A), (8, 0xA5), (15, 0x5A), (15, 0xA5), (9, 0x5A), (6, 0xA5)):
            for null in (False, True):
                with ran(only=[family], **{family: 1}):
                    check_mom(x, batch, codec, esz, D, chunk_len, mask, W, ref, (codec, esz, D, family, W, ops, null), want, ops, byte, null_unselected=null)
            if not ops & 8:
                with ran(only=[family], **{family: 1}):
                    check_mom(x, batch, codec, esz, D, chunk_len, mask, W, 0xFFFFFFFF, (codec, esz, D, family, W, ops, "no such column"), want, ops, byte)


@pytest.mark.parametrize("codec,esz,D,chunk_len,family", [
    ("xff", 2, 8, 8 * 650, "dec_fast"),           # R = 650: 2 rows in the last mask byte, MB = 82 is no multiple of 4, a verbatim tail of 10 rows
    ("delta", 1, 16, 16 * 203, "dec_fast"),       # R = 203, MB = 26
    ("delta", 2, 3, 3 * 333, "dec_generic"),      # (chunks of 1 998 bytes: no whole 16-byte pieces)
    ("xff", 1, 2, 2 * 1001, "dec_generic"),
])
def test_moments_rows_ignores_rows_that_do_not_exist(sz, oracle, no_fast, codec, esz, D, chunk_len, family):
    """every bit set -- on the short chunk's missing rows and on rows >= R in the last byte too -- counts and sums the existing rows
    alone, as no mask at all does; and the mask at an odd address with a short last dword (the read-ahead window, byte by byte)"""
    rng = np.random.default_rng(chunk_len)
    R, MB = fm.geometry(chunk_len, D)
    assert R % 8 and MB % 4
    nchunks = 5
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    ones = np.full((nchunks, MB), 0xFF, np.uint8)
    half = np.packbits(rng.random((nchunks, MB * 8)) < 0.5, axis=1, bitorder="little")
    ref = D - 1
    for fam, fml in ((0, family), (1, "dec_generic")):
        no_fast(fam)
        for W in (8, 64, MB * 8):
            want = mm.moments_rows(x, chunk_len, D, None, W, ref)
            assert int(want["count"].sum()) == x.size // D
            with ran(only=[fml], **{fml: 1}):
                check_mom(x, batch, codec, esz, D, chunk_len, None, W, ref, (codec, D, fml, W, "no mask"), want)
            for shift in (0, 1, 3):
                with ran(only=[fml], **{fml: 2}):
                    check_mom(x, batch, codec, esz, D, chunk_len, ones, W, ref, (codec, D, fml, W, shift, "every bit"), want, mask_shift=shift)
                    check_mom(x, batch, codec, esz, D, chunk_len, half, W, ref, (codec, D, fml, W, shift, "p=1/2"), mask_shift=shift)


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [
    ("xff", 2, 8, 5120, 0),       # decode_fast
    ("delta", 1, 80, 10240, 0),   # decode_fast, two columns a lane
    ("xff", 2, 8, 5120, 1),       # decode_kernel (NO_FAST)
    ("delta", 1, 1, 1024, 0),     # decode_kernel, low-dimension layout
])
def test_moments_rows_damaged_chunk(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
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
    ref = D // 2
    batch.data[off + 6] = hdr[0] ^ 0x5                  # the header's ndims field
    for W in (32, MB * 8):
        check_mom(x, batch, codec, esz, D, chunk_len, mask, W, ref, (codec, D, fam, W), skip_chunk=bad)
    ops = ("count", "sum", "sumsq", "cross")
    with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):
        cd.moments_rows(batch, mask_t, 32, ref=ref, ops=ops, per_chunk=True, check=True)
    cd.moments_rows(batch, mask_t, 32, ref=ref, ops=ops, per_chunk=True, check=False)     # no error without the check
    batch.data[off + 6] = hdr[0]
    got = cd.moments_rows(batch, mask_t, 32, ref=ref, ops=ops, per_chunk=True)            # repaired: no error, and exact
    want = mm.moments_rows(x, chunk_len, D, mask, 32, ref)
    for k in ops:
        assert np.array_equal(got[k].cpu().numpy().astype(np.uint64), want[k].astype(np.uint64)), k


@pytest.mark.parametrize("codec,esz,D,chunk_len,W,nchunks", [
    ("xff", 2, 8, 5120, 64, 6),            # W divides R = 640
    ("xff", 2, 8, 5120, 640, 6),           # W = R
    ("delta", 1, 8, 4096, 2048, 9),        # W = 4 R: the fold, with a partial last window
    ("delta", 1, 1, 1024, 3072, 10),       # univariate, W = 3 R
    ("delta", 2, 3, 300, 500, 12),         # R = 100 is no multiple of 8: one kernel window of 104 rows a chunk
])
def test_moments_rows_python_global_windows(sz, oracle, codec, esz, D, chunk_len, W, nchunks):
    import torch
    rng = np.random.default_rng(W + D)
    x = gen_data("walk", rng, short_batch(nchunks, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    R, MB = fm.geometry(chunk_len, D)
    bits = rng.random((nchunks, MB * 8)) < 0.3
    bits[nchunks // 2] = False                               # a chunk without a selected row: empty windows
    mask = np.packbits(bits, axis=1, bitorder="little")
    mask_t = torch.from_numpy(mask).cuda()
    ref = D - 1
    ints = ("count", "sum", "sumsq", "cross")
    got = cd.moments_rows(batch, mask_t, W, ref=ref, ops=ints + ("mean",))
    want = mm.global_windows(x, chunk_len, D, mask, W, ref)
    for k in ints:
        g = got[k].cpu().numpy()
        assert got[k].dtype == torch.int64 and g.shape == want[k].shape, k
        assert np.array_equal(g, want[k]), k
    mean = got["mean"].cpu().numpy()
    empty = want["count"] == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        assert mean.dtype == np.float64 and np.all(np.isnan(mean[empty])) and np.array_equal(mean[~empty], (want["sum"] / want["count"][:, None])[~empty])
    if W <= R:
        assert empty.any()
    sub = cd.moments_rows(batch, mask_t, W, ops="sumsq")                     # ops as a plain string
    assert list(sub) == ["sumsq"] and torch.equal(sub["sumsq"], got["sumsq"])
    dflt = cd.moments_rows(batch, mask_t, W)
    assert sorted(dflt) == ["count", "sum", "sumsq"]
    one = cd.moments_rows(batch, mask_t, ref=ref, ops=ints, per_chunk=True)  # window_rows=None: one window a chunk
    want1 = mm.moments_rows(x, chunk_len, D, mask, MB * 8, ref)
    assert one["count"].shape == (nchunks, 1) and one["cross"].shape == (nchunks, 1, D)
    for k in ints:
        assert np.array_equal(one[k].cpu().numpy().astype(np.uint64), want1[k].astype(np.uint64)), k
    every = cd.moments_rows(batch, window_rows=W, ref=ref, ops=ints)         # mask=None: every existing row
    want_all = mm.global_windows(x, chunk_len, D, None, W, ref)
    for k in ints:
        assert np.array_equal(every[k].cpu().numpy(), want_all[k]), k
    assert int(every["count"].sum().item()) == x.size // D


def test_moments_where_python(sz, oracle):
    import torch
    codec, esz, D, chunk_len = "xff", 2, 8, 5120
    rng = np.random.default_rng(21)
    x = gen_data("walk", rng, short_batch(6, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    ints = ("count", "sum", "sumsq", "cross")
    for name, mode, lo, hi, _ in sets[:2]:                 # the band (ALL) and the alarm (ANY)
        mask, cnt = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
        for W in (64, 640, 1280):
            with ran(only=["dec_fast"], dec_fast=2):       # the filter launch and the moments launch
                got = cd.moments_where(batch, list(map(int, lo)), list(map(int, hi)), mode="all" if mode == fm.ALL else "any", window_rows=W,
                                       ref=3, ops=ints)
            f = cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), mode="all" if mode == fm.ALL else "any")
            two = cd.moments_rows(batch, f["mask"], W, ref=3, ops=ints)
            want = mm.global_windows(x, chunk_len, D, mask, W, 3)
            assert int(want["count"].sum()) == int(cnt.sum()) > 0
            for k in ints:
                assert torch.equal(got[k], two[k]), (name, W, k)
                assert np.array_equal(got[k].cpu().numpy(), want[k]), (name, W, k)
    none = cd.moments_where(batch, 1, 0)                   # an empty interval: no row, one window a chunk
    assert int(none["count"].sum().item()) == 0 and bool((none["sumsq"] == 0).all()) and none["count"].shape == (6,)
    f = cd.filter_rows(batch, 0, 65535)
    with pytest.raises(ValueError):
        cd.moments_rows(batch, f["mask"][:, :-1])
    with pytest.raises(ValueError):
        cd.moments_rows(batch, f["mask"], 24)              # R = 640: neither a multiple nor a divisor of 24
    with pytest.raises(ValueError):
        cd.moments_rows(batch, f["mask"], 64, ops=("median",))
    for op in ("cross", "cov", "corr"):
        with pytest.raises(ValueError, match="ref"):
            cd.moments_rows(batch, f["mask"], 64, ops=(op,))           # no reference column
    with pytest.raises(ValueError):
        cd.moments_rows(batch, f["mask"], 64, ref=8, ops=("cross",))
    with pytest.raises(ValueError):
        cd.moments_rows(batch, f["mask"], 64, ops=("var",), ddof=2)
    assert cd.moments_rows(batch, f["mask"], 24, per_chunk=True)["count"].shape == (6, 27)
    ragged = sz.ChunkedCodec("delta", 1, 80, 1024, device="cuda:0")        # 1 024 elements are no whole rows of 80
    rb = ragged.compress(torch.randint(0, 255, (1024 * 4,), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):
        ragged.moments_rows(rb, torch.zeros((4, 2), dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(ValueError):
        ragged.moments_where(rb, 0, 100)


def derived_batch(rng, rows, D):
    """uint16 x 8: columns 0 and 1 identical, column 2 constant, column 3 = 65535 - column 4, the rest walks; rows 128 .. 191 (window 2
    of 64 rows) hold 65535 or 65534 alone in the columns that vary -- where n Q - S^2 in float64 fails"""
    assert D == 8
    x = np.mod(np.cumsum(rng.integers(-300, 301, size=(rows, D)), axis=0) + rng.integers(0, 65536, size=(1, D)), 65536)
    x[128:192] = 65534 + rng.integers(0, 2, size=(64, D))
    x[:, 1] = x[:, 0]
    x[:, 2] = 4660
    x[:, 3] = 65535 - x[:, 4]
    return x.astype(np.uint16).ravel()


def test_moments_derived_values(sz, oracle):
    """mean / var / std / cov / corr against the model's exact rationals rounded to float64, window by window and column by column.

    u = 2^-53.  var and cov: |got - exact| <= 6 u (|exact| + 1).  moments_rows forms A - B with A = fl(fl(C) / n') and B = fl(fl(r / n)
    fl(r' / n')) <= 1: A carries two roundings (the conversion of C and the division; n, r and n' are exact in float64), B three, the
    subtraction one, and |A| <= |exact| + 1 -- six roundings of quantities no larger than |exact| + 1.  std is the rounded root of
    that var: std^2 = var (1 + 2 u), so |std^2 - exact var| <= 6 u (exact + 1) + 2 u var <= 8 u (exact + 1), checked on the exact
    square of the returned float.  corr = c / (vx vy)^(1/2) with v = min(vx, vy): each variance carries 6 u (v_i + 1), a relative
    error of at most 6 u (1 + 1 / v); the covariance 6 u (|c| + 1) with |c| <= (vx vy)^(1/2) and that root >= v, the same 6 u (1 +
    1 / v) of the quotient; the product and its root add (2 * 6 (1 + 1 / v) + 1) / 2 + 1 roundings, the division one more: (12 (1 +
    1 / v) + 3) u in all -- 27 u where both variances are >= 1, asserted as 32 u there, and the formula itself below 1.  The returned
    values are not clamped, so |corr| <= 1 + that bound is a check of its own.  mean: one division of exact operands (S < 2^53 here),
    |got - exact| <= u |exact|."""
    import torch
    codec, esz, D, chunk_len, W = "xff", 2, 8, 8 * 640, 64
    rng = np.random.default_rng(77)
    nchunks = 3
    rows = nchunks * 640 - 200
    x = derived_batch(rng, rows, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    MB = 80
    bits = rng.random((nchunks, MB * 8)) < 0.7
    bits[:, 128:192] = True                                 # the all-65534/65535 window in full
    bits[1, 64:128] = False                                 # an empty window
    bits[1, 192:256] = False
    bits[1, 200] = True                                     # a window of one row: n <= ddof at ddof = 1
    mask = np.packbits(bits, axis=1, bitorder="little")
    mask_t = torch.from_numpy(mask).cuda()
    tested = {"empty": 0, "one row": 0, "corr": 0}
    for ref in (0, 4, 6):
        ints = mm.global_windows(x, chunk_len, D, mask, W, ref)
        for ddof in (0, 1):
            with ran(only=["dec_fast"], dec_fast=1):
                got = cd.moments_rows(batch, mask_t, W, ref=ref, ops=("mean", "var", "std", "cov", "corr"), ddof=ddof)
            got = {k: v.cpu().numpy() for k, v in got.items()}
            assert all(v.dtype == np.float64 and v.shape == ints["sum"].shape for v in got.values())
            for w in range(ints["count"].size):
                n = int(ints["count"][w])
                tested["empty"] += n == 0
                tested["one row"] += n == 1
                for d in range(D):
                    S, Q, P = int(ints["sum"][w, d]), int(ints["sumsq"][w, d]), int(ints["cross"][w, d])
                    e = mm.exact_derived(n, S, Q, P, int(ints["sum"][w, ref]), int(ints["sumsq"][w, ref]), ddof)
                    msg = (ref, ddof, w, d, n)
                    if e["mean"] is None:
                        assert np.isnan(got["mean"][w, d]), msg
                    else:
                        assert abs(Fraction(got["mean"][w, d]) - e["mean"]) <= Fraction(U) * abs(e["mean"]), msg
                    for k in ("var", "cov"):
                        if e[k] is None:
                            assert np.isnan(got[k][w, d]), (k,) + msg
                        else:
                            assert abs(Fraction(got[k][w, d]) - e[k]) <= 6 * Fraction(U) * (abs(e[k]) + 1), (k, got[k][w, d], float(e[k])) + msg
                    if e["var"] is None:
                        assert np.isnan(got["std"][w, d]), msg
                    else:
                        assert abs(Fraction(got["std"][w, d]) ** 2 - e["var"]) <= 8 * Fraction(U) * (e["var"] + 1), msg
                    if e["corr2"] is None:
                        assert np.isnan(got["corr"][w, d]), msg
                    else:
                        vx, vy = Fraction(n * Q - S * S, n * n), mm.exact_derived(n, int(ints["sum"][w, ref]), int(ints["sumsq"][w, ref]))["var"]
                        bound = corr_bound(vx, vy)
                        assert abs(got["corr"][w, d] - mm.corr_float(e)) <= bound, (got["corr"][w, d], mm.corr_float(e)) + msg
                        assert abs(got["corr"][w, d]) <= 1.0 + bound, msg
                        tested["corr"] += vx >= 1 and vy >= 1
    assert all(v > 0 for v in tested.values()), tested
    # one window of 1 720 rows that hold 65535 or 65534 alone: n Q and S^2 pass 2^53 and n Q - S^2 in float64 loses the variance's
    # low bits -- the pivot does not
    y = (65534 + rng.integers(0, 2, size=(rows, D))).astype(np.uint16).ravel()
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, y, False)
    ints = mm.global_windows(y, chunk_len, D, None, 3 * 640, 1)
    assert ints["count"].tolist() == [rows]
    with ran(only=["dec_fast"], dec_fast=1):
        got = cd.moments_rows(batch, window_rows=3 * 640, ref=1, ops=("var", "cov", "corr"))
    naive_fails = 0
    for d in range(D):
        n, S, Q = rows, int(ints["sum"][0, d]), int(ints["sumsq"][0, d])
        e = mm.exact_derived(n, S, Q, int(ints["cross"][0, d]), int(ints["sum"][0, 1]), int(ints["sumsq"][0, 1]))
        assert abs(Fraction(float(got["var"][0, d])) - e["var"]) <= 6 * Fraction(U) * (e["var"] + 1), d
        assert abs(Fraction(float(got["cov"][0, d])) - e["cov"]) <= 6 * Fraction(U) * (abs(e["cov"]) + 1), d
        vy = mm.exact_derived(n, int(ints["sum"][0, 1]), int(ints["sumsq"][0, 1]))["var"]
        assert abs(float(got["corr"][0, d]) - mm.corr_float(e)) <= corr_bound(e["var"], vy), d      # (variances of about 1/4)
        naive = (float(n) * float(Q) - float(S) * float(S)) / (float(n) * float(n))
        naive_fails += abs(Fraction(naive) - e["var"]) > 6 * Fraction(U) * (e["var"] + 1)
    assert naive_fails > 0


def test_corr_python(sz, oracle):
    """corr on 8 columns of which two are identical, one is constant and one is 65535 - another: 1, NaN and -1 in the right places, a
    symmetric matrix and a unit diagonal where defined"""
    import torch
    codec, esz, D, chunk_len, W = "xff", 2, 8, 8 * 640, 640
    rng = np.random.default_rng(78)
    x = derived_batch(rng, 3 * 640 - 200, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    with ran(only=["dec_fast"], dec_fast=D):               # one launch per reference column
        m = cd.corr(batch, window_rows=W).cpu().numpy()
    assert m.shape == (3, D, D) and m.dtype == np.float64
    assert np.array_equal(m, np.transpose(m, (0, 2, 1)), equal_nan=True)
    varies = [d for d in range(D) if d != 2]
    for w in range(3):
        assert np.all(np.isnan(m[w, 2, :])) and np.all(np.isnan(m[w, :, 2]))          # the constant column
        assert np.all(np.abs(m[w, varies, varies] - 1.0) <= 32 * U) and np.all(np.abs(m[w][~np.isnan(m[w])]) <= 1.0 + 32 * U)
        assert abs(m[w, 0, 1] - 1.0) <= 32 * U and abs(m[w, 3, 4] + 1.0) <= 32 * U
        ints = {r: mm.global_windows(x, chunk_len, D, None, W, r) for r in varies}
        for i in varies:
            for j in varies:
                g = ints[j]
                e = mm.exact_derived(g["count"][w], g["sum"][w, i], g["sumsq"][w, i], g["cross"][w, i], g["sum"][w, j], g["sumsq"][w, j])
                assert abs(m[w, i, j] - mm.corr_float(e)) <= 32 * U, (w, i, j)          # (every variance here is far above 1)
    with ran(only=["dec_fast"], dec_fast=3):
        sub = cd.corr(batch, cols=[4, 0, 3], window_rows=W).cpu().numpy()
    assert np.array_equal(sub, m[:, [4, 0, 3]][:, :, [4, 0, 3]])
    f = cd.filter_rows(batch, 0, 65535)
    assert np.array_equal(cd.corr(batch, cols=[0, 5], mask=f["mask"], window_rows=W).cpu().numpy(), m[:, [0, 5]][:, :, [0, 5]])
    with pytest.raises(ValueError):
        cd.corr(batch, cols=[8])


def test_moments_rows_headline_shape(sz, oracle):
    """64 chunks of the headline shape (uint16 x 8, FIRE, 10 KB chunks), filter_rows' band mask from the device, W = 64, all four ops"""
    codec, esz, D, chunk_len, nchunks, W, ref = "xff", 2, 8, 5120, 64, 64, 3
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
        want = check_mom(x, batch, codec, esz, D, chunk_len, mask, W, ref, ("headline",))
    assert np.array_equal(want["count"].sum(axis=1), cnt)
    with ran(only=["dec_fast"], dec_fast=1):
        got = cd.moments_rows(batch, f["mask"], W, ref=ref, ops=("count", "sum", "sumsq", "cross"), per_chunk=True)
    for k in ("count", "sum", "sumsq", "cross"):
        assert np.array_equal(got[k].cpu().numpy().astype(np.uint64), want[k].astype(np.uint64)), k
