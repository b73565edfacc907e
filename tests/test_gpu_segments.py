"""GPU tests (-m gpu) of segment rows (sprintz_mi355x_segment_count / _segment_rows, ChunkedCodec.segment_rows / segments_where /
sessions): per run of rows a mask names -- or per stretch between two set bits -- its start, its length and min / max / sum, placed behind
the chunk's base, in decode_fast.h and decode_kernel.h.  The expected value is always tests/segment_model.py applied to the ORIGINAL
input, never a decode by the library, and every comparison is exact.  Every launch's kernel family is asserted, every output lies in a
sentinel-filled buffer with 1 024 entries of padding that must keep the sentinel, rets[nchunks] must stay untouched, and the parity,
mapping and placement batches end in a short last chunk of whole rows.  What the masks must reach is asserted without a device in
tests/test_segments_cpu.py."""
import ctypes as C
import zlib

import numpy as np
import pytest

import filter_model as fm
import segment_model as sgm
from dispatch import counts as dispatch_counts
from dispatch import ran
from harness import DTYPES
from drive_tables import (BAD, DAMAGE_IDS, DAMAGE_SHAPES, FIRE_IDS, FIRE_SHAPES, ROWOP_CASES, ROWOP_IDS, damaged, fire_batch, fire_legs, legs,
                          masks_for, rowop_batch, three_of_8, truncated)  # noqa: F401  (fixtures)
from fixtures import chunks_per_group, no_fast, sentinel, sz  # noqa: F401  (fixtures)
from rowdata import FAST_SHAPES, PARITY_FAST, gen_data, lowdim, make_batch, masked_parity_cases as parity_cases, parity_masks, rows_for, short_batch
from streams import OLD, options

pytestmark = pytest.mark.gpu

PAD = 1024                      # entries behind every output that must keep the sentinel
MODES = ((sgm.RUNS, "runs"), (sgm.SPLITS, "splits"))
OPS = {"min": sgm.MIN, "max": sgm.MAX, "sum": sgm.SUM, "rows": sgm.ROWS, "start": sgm.START}
WIDTH = {"sum": 8, "rows": 4, "start": 8}


def codec_id(codec):
    from sprintz_amd import _lib
    return _lib.CODEC_DELTA if codec == "delta" else _lib.CODEC_XFF


def device_mask(mask, shift=0):
    """the mask `shift` bytes into a buffer of 0xFF bytes, 16 more behind it -> (tensor, pointer)"""
    import torch
    flat = np.ascontiguousarray(mask, np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.full(shift, 0xFF, np.uint8), flat, np.full(16, 0xFF, np.uint8)])).cuda()
    return t, t.data_ptr() + shift


def run_count(mask, n, chunk_len, D, mode, lens=None, shift=0, stream=None):
    """sprintz_mi355x_segment_count on a sentinel-filled buffer of n + PAD entries -> uint32 [n]"""
    import torch
    from sprintz_amd import _lib
    counts = torch.full((n + PAD,), -77, dtype=torch.int32, device="cuda")
    mask_t, mptr = device_mask(mask, shift)
    lens_t = None if lens is None else torch.from_numpy(np.asarray(lens, np.int64)).cuda()
    st = stream if stream is not None else torch.cuda.current_stream()
    before = dispatch_counts()
    _lib.check(_lib.segment_count(mptr, n, chunk_len, D, mode, lens_t.data_ptr() if lens_t is not None else None, counts.data_ptr(), C.c_void_p(st.cuda_stream)))
    assert dispatch_counts() == before, "segment_count counts under no kernel family"
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    assert np.all(c[n:] == -77), "counts written past nchunks"
    return c[:n].view(np.uint32)


def run_seg(batch, codec, esz, D, chunk_len, mask, mode, bases, capacity, ops=31, byte=0x5A, general=False, mask_shift=0, null_unselected=False, stream=None):
    """the C entry point on sentinel-filled outputs of capacity + PAD entries -> ({op: numpy incl. padding}, rets [nchunks])"""
    import torch
    from sprintz_amd import _lib
    n = batch.nchunks
    m = capacity + PAD
    elem = np.full(m * D, sentinel(esz, byte), DTYPES[esz]).view(np.int8 if esz == 1 else np.int16)
    bufs = {
        "min": torch.from_numpy(elem.copy()).cuda(), "max": torch.from_numpy(elem.copy()).cuda(),
        "sum": torch.from_numpy(np.full(m * D, sentinel(8, byte), np.uint64).view(np.int64)).cuda(),
        "rows": torch.from_numpy(np.full(m, sentinel(4, byte), np.uint32).view(np.int32)).cuda(),
        "start": torch.from_numpy(np.full(m, sentinel(8, byte), np.uint64).view(np.int64)).cuda(),
    }
    rets_t = torch.full((n + 1,), -77, dtype=torch.int64, device="cuda")
    mask_t, mptr = device_mask(mask, mask_shift)
    bases_t = torch.from_numpy(np.ascontiguousarray(bases, np.int64)).cuda()
    st = stream if stream is not None else torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())

    def ptr(k):
        return None if null_unselected and not ops & OPS[k] else bufs[k].data_ptr()
    _lib.check(_lib.segment_rows(codec_id(codec), esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, chunk_len, D, mptr, mode,
                                 bases_t.data_ptr(), int(capacity), ops, _lib.QUERY_GENERAL_LAYOUT if general else 0,
                                 ptr("min"), ptr("max"), ptr("sum"), ptr("rows"), ptr("start"), rets_t.data_ptr(), C.c_void_p(st.cuda_stream)))
    torch.cuda.synchronize()
    r = rets_t.cpu().numpy()
    assert r[n] == -77, "rets written past nchunks"
    got = {"min": bufs["min"].cpu().numpy().view(DTYPES[esz]), "max": bufs["max"].cpu().numpy().view(DTYPES[esz]),
           "sum": bufs["sum"].cpu().numpy().view(np.uint64), "rows": bufs["rows"].cpu().numpy().view(np.uint32),
           "start": bufs["start"].cpu().numpy().view(np.uint64)}
    return got, r[:n]


def check_seg(x, batch, codec, esz, D, chunk_len, mask, mode, msg, model=None, bases=None, capacity=None, ops=31, byte=0x5A, skip_chunk=None, **kw):
    """every output -- the selected ones entry by entry, places nobody writes and the padding at the sentinel, the unselected ones untouched
    -- and rets against the model.  bases / capacity default to the counts' exclusive prefix sum and their total.  skip_chunk: a damaged
    chunk, of which only the places [bases[c], bases[c] + the starts of its mask over rows 0 .. R-1) are unspecified"""
    model = sgm.segment_rows(x, chunk_len, D, mask, mode) if model is None else model
    cnt = model["counts"].astype(np.int64)
    bases = np.cumsum(cnt) - cnt if bases is None else np.asarray(bases, np.int64)
    capacity = int(cnt.sum()) if capacity is None else int(capacity)
    if skip_chunk is not None:                             # the model's places for the damaged chunk are not the call's: they are skipped below
        span = int(sgm.segment_count(mask, chunk_len, D, mode)[skip_chunk])
        assert span >= cnt[skip_chunk]
    want = sgm.placed(model, bases, capacity, D, DTYPES[esz], byte, PAD)
    got, rets = run_seg(batch, codec, esz, D, chunk_len, mask, mode, bases, capacity, ops, byte, **kw)
    lens = np.array(fm.chunk_counts(x.size, chunk_len))
    keep_c = np.arange(batch.nchunks) != (-1 if skip_chunk is None else skip_chunk)
    assert np.array_equal(rets[keep_c], lens[keep_c]), ("rets",) + msg
    keep = np.ones(capacity + PAD, bool)
    if skip_chunk is not None:
        assert rets[skip_chunk] < 0, ("rets of the damaged chunk",) + msg
        keep[int(bases[skip_chunk]):min(int(bases[skip_chunk]) + span, capacity)] = False
    for k in OPS:
        sent = sentinel(WIDTH.get(k, esz), byte)
        per = D if k in ("min", "max", "sum") else 1
        g, w = got[k].reshape(-1, per), want[k].reshape(-1, per)
        if ops & OPS[k]:
            bad = np.flatnonzero((g != w).any(axis=1) & keep)
            assert bad.size == 0, (k, "first wrong place", int(bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist()) + msg
        else:
            assert np.all(g == sent), (k, "an unselected output was written") + msg
    return model


def all_masks(rng, x, chunk_len, esz, D):
    return parity_masks(rng, x, chunk_len, esz, D) + sgm.extra_masks(rng, x.size, chunk_len, D)


@pytest.mark.parametrize("codec,esz,D,shape,data", parity_cases())
def test_segment_rows_parity(sz, oracle, no_fast, codec, esz, D, shape, data):
    """both layouts of the low-dimension shapes x nineteen masks x both rules x both families: every output equals the model, and
    segment_count -- with the true lengths: the model's counts and the places written; without lengths: the starts over R rows"""
    rng = np.random.default_rng(zlib.crc32(f"segments{codec}{esz}{D}{shape}{data}".encode()))
    R = rows_for(shape, D)
    chunk_len = R * D
    x = gen_data(data, rng, short_batch(5, chunk_len, D), esz, D)
    lens = fm.chunk_counts(x.size, chunk_len)
    masks = all_masks(rng, x, chunk_len, esz, D)
    models = {(name, mode): sgm.segment_rows(x, chunk_len, D, mask, mode) for name, mask in masks for mode, _ in MODES}
    for name, mask in masks:
        for mode, _ in MODES:
            want = models[(name, mode)]["counts"]
            assert np.array_equal(run_count(mask, 5, chunk_len, D, mode, lens), want), ("count", name, mode)
            assert np.array_equal(run_count(mask, 5, chunk_len, D, mode), sgm.segment_count(mask, chunk_len, D, mode)), ("count over R rows", name, mode)
    for general in ((False, True) if lowdim(esz, D) else (False,)):
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, general)
        first = "dec_fast" if (esz, D, general) in PARITY_FAST else "dec_generic"
        for fam, family in ((0, first), (1, "dec_generic")):
            if fam == 1 and first == "dec_generic":
                continue                                   # (the same kernel again)
            no_fast(fam)
            for name, mask in masks:
                for mode, _ in MODES:
                    with ran(only=[family], **{family: 1}):
                        check_seg(x, batch, codec, esz, D, chunk_len, mask, mode, (codec, esz, D, shape, data, general, family, name, mode),
                                  models[(name, mode)], general=general)
    assert int(models[("no row", sgm.RUNS)]["counts"].sum()) == 0 and models[("no row", sgm.SPLITS)]["counts"].tolist() == [1] * 5
    assert models[("every bit", sgm.RUNS)]["rows"].tolist() == [n // D for n in lens]


@pytest.mark.parametrize("codec,esz,D,chunk_len", FAST_SHAPES)
def test_segment_rows_fast_mappings(sz, oracle, no_fast, codec, esz, D, chunk_len):
    """each of decode_fast.h's lane mappings on chunks it takes -- 4 .. 64 lanes a chunk, 1 / 2 / 4 columns a lane -- under the ruler, p = 1/2
    and band masks, both rules; the generic kernel on the same batch"""
    rng = np.random.default_rng(zlib.crc32(f"segfast{codec}{esz}{D}".encode()))
    x = gen_data("walk", rng, short_batch(4, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    masks = dict(all_masks(rng, x, chunk_len, esz, D))
    for name in ("ruler", "p=1/2", "band"):
        for mode, _ in MODES:
            model = None
            for fam, family in ((0, "dec_fast"), (1, "dec_generic")):
                no_fast(fam)
                with ran(only=[family], **{family: 1}):
                    model = check_seg(x, batch, codec, esz, D, chunk_len, masks[name], mode, (codec, esz, D, family, name, mode), model)
            assert int(model["counts"].sum()) > 4


# ------------------------------------------------------------------ the drives

@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_segment_rows_over_runs(sz, oracle, no_fast, chunks_per_group, codec, w, D, kind):
    """runs of 1 .. 16 zero blocks, streams that open with a run and end in one: masks that cut runs (the replay on the constant row),
    masks that leave them whole inside a segment and outside every one (the O(1) step), at one and at three chunks a lane group"""
    cd, batch, data, chunk_len, zero = rowop_batch(sz, oracle, codec, w, D, kind)
    with options(**OLD):
        for name, mask in masks_for(zero, 41)[:3]:
            for mode, _ in MODES:
                model = sgm.segment_rows(data, chunk_len, D, mask, mode)
                for fam, cpg, family in legs(w, D, "aggregate"):
                    no_fast(fam)
                    chunks_per_group(cpg)
                    with ran(only=[family], **{family: 1}):
                        check_seg(data, batch, codec, w // 8, D, chunk_len, mask, mode, (codec, w, D, kind, name, mode, family, cpg), model)


@pytest.mark.parametrize("w,D", list(FIRE_SHAPES), ids=FIRE_IDS)
def test_segment_rows_on_the_fire_drive(sz, oracle, chunks_per_group, w, D):
    """FIRE runs are replayed block by block at frozen extreme coefficients, under both rules"""
    cd, batch, data, chunk_len, nchunks = fire_batch(sz, oracle, w, D)
    mask = three_of_8(nchunks, chunk_len // D)
    for mode, _ in MODES:
        model = sgm.segment_rows(data, chunk_len, D, mask, mode)
        for family, cpg in fire_legs(sz, w, D, chunks_per_group):
            with ran(only=[family], **{family: 1}):
                check_seg(data, batch, "xff", w // 8, D, chunk_len, mask, mode, (w, D, mode, family, cpg), model)


# ------------------------------------------------------------------ placement

PLACE_SHAPES = [("xff", 2, 8, 5120, 0, "dec_fast"), ("delta", 1, 80, 10240, 0, "dec_fast"), ("xff", 1, 3, 3000, 0, "dec_generic"), ("xff", 2, 8, 5120, 1, "dec_generic")]


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam,family", PLACE_SHAPES)
def test_segment_rows_placement(sz, oracle, no_fast, codec, esz, D, chunk_len, fam, family):
    """bases in reverse chunk order with gaps; a capacity below the total, and 0; every op alone with the unselected outputs given and NULL;
    the mask at byte offsets 1 and 3; a stream of its own; a second sentinel"""
    import torch
    no_fast(fam)
    rng = np.random.default_rng(D + fam)
    n = 6
    x = gen_data("walk", rng, short_batch(n, chunk_len, D), esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    mask = dict(sgm.extra_masks(rng, x.size, chunk_len, D))["ruler"]
    lens = fm.chunk_counts(x.size, chunk_len)
    side = torch.cuda.Stream()
    for mode, _ in MODES:
        model = sgm.segment_rows(x, chunk_len, D, mask, mode)
        cnt = model["counts"].astype(np.int64)
        total = int(cnt.sum())
        assert total > 4 * n
        msg = (codec, esz, D, family, mode)
        rev = np.zeros(n, np.int64)                        # chunk n - 1 first, 3 places of nothing between two chunks
        pos = 2
        for c in range(n - 1, -1, -1):
            rev[c] = pos
            pos += int(cnt[c]) + 3
        prefix = np.cumsum(cnt) - cnt
        with ran(only=[family], **{family: 7}):
            check_seg(x, batch, codec, esz, D, chunk_len, mask, mode, msg + ("reverse bases",), model, rev, pos)
            check_seg(x, batch, codec, esz, D, chunk_len, mask, mode, msg + ("capacity below the total",), model, prefix, total - int(cnt[-1]) - 2)
            check_seg(x, batch, codec, esz, D, chunk_len, mask, mode, msg + ("reverse bases, capacity inside",), model, rev, pos // 2)
            check_seg(x, batch, codec, esz, D, chunk_len, mask, mode, msg + ("capacity 0",), model, prefix, 0)
            check_seg(x, batch, codec, esz, D, chunk_len, mask, mode, msg + ("mask + 1",), model, mask_shift=1)
            check_seg(x, batch, codec, esz, D, chunk_len, mask, mode, msg + ("mask + 3",), model, mask_shift=3, byte=0xA5)
            check_seg(x, batch, codec, esz, D, chunk_len, mask, mode, msg + ("side stream",), model, stream=side)
        assert np.array_equal(run_count(mask, n, chunk_len, D, mode, lens, shift=3, stream=side), model["counts"])
        for ops, byte in ((1, 0x5A), (2, 0xA5), (4, 0x5A), (8, 0xA5), (16, 0x5A), (24, 0xA5), (7, 0x5A)):
            for null in (False, True):
                with ran(only=[family], **{family: 1}):
                    check_seg(x, batch, codec, esz, D, chunk_len, mask, mode, msg + (ops, null), model, ops=ops, byte=byte, null_unselected=null)


# ------------------------------------------------------------------ damage

@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_damaged_chunk_in_a_group_segment_rows(sz, damaged, codec, w, D):
    """a chunk rejected at its header in the middle of a lane group of three: its rets entry is negative, only its own places differ"""
    cd, batch, data, chunk_len, mask = damaged(codec, w, D)
    for mode, _ in MODES:
        with ran(only=["dec_fast"], dec_fast=1):
            check_seg(data, batch, codec, w // 8, D, chunk_len, mask, mode, (codec, w, D, mode), skip_chunk=BAD)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_truncated_chunk_in_a_group_segment_rows(sz, truncated, codec, w, D):
    """a chunk found damaged only at its end, while a segment is open in the registers: the next chunk of the group starts clean"""
    cd, batch, data, chunk_len, mask = truncated(codec, w, D)
    every = np.full_like(mask, 0xFF)                       # one segment a chunk: open from row 0 to the damage
    for m in (mask, every):
        for mode, _ in MODES:
            with ran(only=["dec_fast"], dec_fast=1):
                check_seg(data, batch, codec, w // 8, D, chunk_len, m, mode, (codec, w, D, mode), skip_chunk=BAD)


# ------------------------------------------------------------------ refusals

def test_segment_refusals(sz, oracle):
    """each SPRINTZ_E_INVALID / _UNSUPPORTED of both entry points, with nothing launched"""
    import torch
    from sprintz_amd import _lib
    codec, esz, D, chunk_len, n = "xff", 2, 8, 5120, 3
    rng = np.random.default_rng(3)
    x = gen_data("walk", rng, n * chunk_len, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    MB = chunk_len // D // 8
    mask = torch.zeros(n * MB + 16, dtype=torch.uint8, device="cuda")
    bases = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    big = torch.zeros(4096, dtype=torch.int64, device="cuda")
    rets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(n + 2, dtype=torch.int32, device="cuda")
    p = big.data_ptr()
    good = dict(codec=_lib.CODEC_XFF, esz=esz, comp=batch.data.data_ptr(), offs=batch.offsets.data_ptr(), n=n, chunk_len=chunk_len, D=D, mask=mask.data_ptr(),
                mode=0, bases=bases.data_ptr(), cap=16, ops=31, flags=0, mn=p, mx=p, sm=p, rows=p, start=p, rets=rets.data_ptr())

    def seg(**kw):
        a = dict(good, **kw)
        return _lib.segment_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["chunk_len"], a["D"], a["mask"], a["mode"], a["bases"], a["cap"], a["ops"],
                                 a["flags"], a["mn"], a["mx"], a["sm"], a["rows"], a["start"], a["rets"], None)

    def cnt(mask_p=mask.data_ptr(), n_=n, chunk_len_=chunk_len, D_=D, mode=0, lens=None, counts_p=counts.data_ptr()):
        return _lib.segment_count(mask_p, n_, chunk_len_, D_, mode, lens, counts_p, None)
    before = dispatch_counts()
    inv, uns = _lib.E_INVALID, _lib.E_UNSUPPORTED
    for kw, code in [(dict(mode=2), inv), (dict(ops=0), inv), (dict(ops=32), inv), (dict(flags=2), inv), (dict(mask=None), inv), (dict(bases=None), inv),
                     (dict(comp=None), inv), (dict(offs=None), inv), (dict(mn=None), inv), (dict(start=None), inv), (dict(rows=None), inv),
                     (dict(mx=p + 1), inv), (dict(sm=p + 4), inv), (dict(rows=p + 2), inv), (dict(start=p + 4), inv), (dict(bases=bases.data_ptr() + 4), inv),
                     (dict(rets=rets.data_ptr() + 4), inv), (dict(chunk_len=5121), inv), (dict(chunk_len=0), inv), (dict(esz=3), inv), (dict(D=0), inv),
                     (dict(codec=_lib.CODEC_DELTA_NORLE), uns), (dict(D=520, chunk_len=5200), uns)]:
        assert seg(**kw) == code, kw
        assert _lib.last_error(), kw
    assert seg(ops=8, mn=None, mx=None, sm=None, start=None, n=0) == 0 and seg(n=0, comp=None, offs=None) == inv
    for kw, code in [(dict(mode=2), inv), (dict(D_=0), inv), (dict(chunk_len_=0), inv), (dict(chunk_len_=5121), inv), (dict(mask_p=None), inv),
                     (dict(counts_p=None), inv), (dict(counts_p=counts.data_ptr() + 2), inv), (dict(lens=rets.data_ptr() + 4), inv)]:
        assert cnt(**kw) == code, kw
        assert "segment_count" in _lib.last_error(), kw
    assert cnt(n_=0, mask_p=None, counts_p=None) == 0
    torch.cuda.synchronize()
    assert dispatch_counts() == before, "a refused call launched a kernel"
    assert _lib.abi_version() == 7


# ------------------------------------------------------------------ Python

def as_np(v, esz):
    import torch
    if v.dtype in (torch.uint8, torch.uint16):
        return v.view(torch.int8 if esz == 1 else torch.int16).cpu().numpy().view(DTYPES[esz])
    return v.cpu().numpy()


def assert_python(got, want, esz, ops, msg):
    assert set(got) == {"start", "rows"} | set(ops), msg
    for k in got:
        g = as_np(got[k], esz)
        assert g.shape == want[k].shape and np.array_equal(g, want[k]), (k,) + msg


def test_segment_rows_python(sz, oracle):
    """segment_rows, segments_where (with and without zones) and sessions against the model of the batch taken as one chunk, on 16 chunks"""
    import torch
    codec, esz, D, chunk_len, n = "xff", 2, 8, 8 * 104, 16
    R = chunk_len // D
    rng = np.random.default_rng(16)
    x = gen_data("walk", rng, short_batch(n, chunk_len, D), esz, D).reshape(-1, D).copy()
    x[:, 0] = (np.arange(x.shape[0]) // 39 % 5) * 100                              # a state column: a change every 39 rows -- at row 0 of every third chunk (8 * 39 = 3 * 104)
    x[R * 3 - 5:R * 5 + 9, 1] = 60000                                              # an excursion of column 1 over three chunks
    x = x.ravel()
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    masks = dict(sgm.extra_masks(rng, x.size, chunk_len, D))
    for name in ("ruler", "last row and row 0", "p=1/2, padding set"):
        mask_t = torch.from_numpy(masks[name]).cuda()
        for mode, mname in MODES:
            for min_rows in (1, 3):
                got = cd.segment_rows(batch, mask_t, mode=mname, min_rows=min_rows)
                assert_python(got, sgm.segment_rows_one_chunk(x, chunk_len, D, masks[name], mode, min_rows), esz, ("min", "max", "sum"), (name, mname, min_rows))
        only = cd.segment_rows(batch, mask_t, ops="max")
        assert_python(only, {k: v for k, v in sgm.segment_rows_one_chunk(x, chunk_len, D, masks[name], sgm.RUNS).items() if k in ("start", "rows", "max")}, esz, ("max",), (name,))
        assert got["start"].dtype == torch.int64 and got["rows"].dtype == torch.int64 and got["sum"].dtype == torch.int64 and got["min"].dtype == cd.dtype
    # segments_where: the excursion of column 1, one segment over three chunks, with and without the zone map
    lo, hi = [0] * D, [65535] * D
    lo[1] = 60000
    want_mask = fm.filter_rows(x, chunk_len, D, np.array(lo), np.array(hi), fm.ALL)[0]
    want = sgm.segment_rows_one_chunk(x, chunk_len, D, want_mask, sgm.RUNS)
    assert (R * 3 - 5) in want["start"].tolist() and int(want["rows"][want["start"].tolist().index(R * 3 - 5)]) >= 2 * R + 14
    zones = cd.zone_map(batch)
    for z in (None, zones):
        assert_python(cd.segments_where(batch, lo, hi, zones=z), want, esz, ("min", "max", "sum"), ("segments_where", z is not None))
    long_ = cd.segments_where(batch, lo, hi, min_rows=2 * R, ops=("max", "sum"))
    assert_python(long_, {k: v for k, v in sgm.segment_rows_one_chunk(x, chunk_len, D, want_mask, sgm.RUNS, 2 * R).items() if k != "min"}, esz, ("max", "sum"), ("min_rows",))
    assert long_["start"].numel() >= 1
    # sessions: the stretches between the changes of column 0
    col = x.reshape(-1, D)[:, 0]
    change = np.zeros(n * R, bool)
    change[1:col.size] = col[1:] != col[:-1]
    smask = sgm.pack_bits(change.reshape(n, R))
    want = sgm.segment_rows_one_chunk(x, chunk_len, D, smask, sgm.SPLITS)
    assert want["rows"].max() == 39 and np.any((want["start"] % R == 0) & (want["start"] > 0))      # a change at a chunk's row 0
    got = cd.sessions(batch, 0)
    assert_python(got, want, esz, ("min", "max", "sum"), ("sessions",))
    assert bool((got["min"][:, 0] == got["max"][:, 0]).all())                      # the state is constant over a session
    assert_python(cd.sessions(batch, 0, ops=("sum",), min_rows=39), {k: v for k, v in sgm.segment_rows_one_chunk(x, chunk_len, D, smask, sgm.SPLITS, 39).items() if k in ("start", "rows", "sum")},
                  esz, ("sum",), ("sessions, min_rows",))
    with pytest.raises(ValueError):
        cd.segment_rows(batch, mask_t, mode="windows")
    with pytest.raises(ValueError):
        cd.segment_rows(batch, mask_t[:, :-1])
    # check=True raises on the damaged batch
    off = int(batch.offsets[5].item())
    keep = batch.data[off + 6].clone()
    batch.data[off + 6] = keep ^ 0x5
    with pytest.raises(sz.SprintzError, match="chunk 5 "):
        cd.segment_rows(batch, mask_t)
    cd.segment_rows(batch, mask_t, check=False)
    batch.data[off + 6] = keep
    cd.segment_rows(batch, mask_t)
