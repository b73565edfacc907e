"""GPU tests (-m gpu): the later row operations -- extrema, moments, histogram and group-by rows, the linear filter and the zone map with
its pruning -- over the two drives, at one and at three chunks a lane group.

Their own tests reach decode_fast.h's delta-run shortcuts (EXT through run_selected_span, LIN with lcarry / lfirst and the first[] store,
MOM, GBY, HIST) with one shape of run: hundreds of flat blocks from a multiple of 8 rows to the chunk's end.  tests/rle_drive.py's batches
put runs of 1 .. 16 blocks on 16 consecutive block indices, open a stream with a run, close runs by a packed block inside a window and
end chunks in a run; tests/fire_drive.py's make every operation replay run blocks at frozen extreme coefficients.  And with
SPRINTZ_OPT_CHUNKS_PER_GROUP above 1 the chunk loop of decode_fast.h has to reset every mode's per-chunk state and reads ahead across
the seam: every case runs at 1 and at 3 (16 chunks: groups of 3, 3, 3, 3, 3 and 1), and once more with a chunk rejected at its header
in the middle of a group -- and, for the modes that keep a window open in registers, with one found damaged only at its end.

Expected values are the numpy models applied to the RAW samples, never a decode by the library; the containers are the ORACLE's; every
launch asserts its kernel family (literals that tests/test_rowop_drive_cpu.py replays through the planner), and every comparison is
exact.  What the batches, masks, binnings and bands below must reach is asserted without a device in tests/test_rowop_drive_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import extrema_model as em
import filter_model as fm
import groupby_model as gbm
import histogram_model as hm
import linear_model as lm
import moments_model as mm
import select_model as sm
import window_model as wm
import zone_model as zm
from drive_tables import (BAD, DAMAGE_IDS, DAMAGE_SHAPES, FIRE_COL, FIRE_IDS, FIRE_SHAPES, GBY_KEY, GBY_TABLES, LIN_COL, NCHUNKS, ROWOP_CASES,
                          ROWOP_IDS, WINDOWS, band_bounds, damaged, fire_batch, fire_change_bounds, fire_legs, fire_patched, fire_windows,
                          gby_binning, hist_binnings, legs, linear_sets, masks_for, refs_for, rowop_batch, three_of_8, truncated, zone_band)  # noqa: F401  (fixtures)
from fixtures import chunks_per_group, no_fast, sentinels, sz  # noqa: F401  (fixtures)
from rowdata import bound_sets
from rowop_runners import assert_zone_map, check_agg, check_ext, check_gby, check_hist, check_mom, raw_linear, run_linear, run_select
from streams import OLD, options
from dispatch import ran

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ what the cases run on: pure functions of the seeded batches, shared with the CPU tier


# ------------------------------------------------------------------ 1 + 2. the RLE drive, at one and at three chunks a lane group

@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_extrema_rows_over_runs(sz, oracle, no_fast, chunks_per_group, codec, w, D, kind):
    """all eight outputs: a run's first selected row in a window is its argmin / argmax and the window's first row, its last the window's last"""
    cd, batch, data, chunk_len, zero = rowop_batch(sz, oracle, codec, w, D, kind)
    with options(**OLD):
        for name, mask in masks_for(zero, 21):
            for W in WINDOWS:
                want = em.extrema_rows(data, chunk_len, D, mask, W)
                for fam, cpg, family in legs(w, D, "extrema"):
                    no_fast(fam)
                    chunks_per_group(cpg)
                    with ran(only=[family], **{family: 1}):
                        check_ext(data, batch, codec, w // 8, D, chunk_len, mask, W, (codec, w, D, kind, name, W, family, cpg), want, ops=255)


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_moments_rows_over_runs(sz, oracle, no_fast, chunks_per_group, codec, w, D, kind):
    """all four sums, the reference column first, in the middle and last"""
    cd, batch, data, chunk_len, zero = rowop_batch(sz, oracle, codec, w, D, kind)
    with options(**OLD):
        for name, mask in masks_for(zero, 22):
            for W in WINDOWS:
                for ref in refs_for(D):
                    want = mm.moments_rows(data, chunk_len, D, mask, W, ref)
                    for fam, cpg, family in legs(w, D, "moments"):
                        no_fast(fam)
                        chunks_per_group(cpg)
                        with ran(only=[family], **{family: 1}):
                            check_mom(data, batch, codec, w // 8, D, chunk_len, mask, W, ref, (codec, w, D, kind, name, W, ref, family, cpg), want)


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_histogram_rows_over_runs(sz, oracle, no_fast, chunks_per_group, codec, w, D, kind):
    cd, batch, data, chunk_len, zero = rowop_batch(sz, oracle, codec, w, D, kind)
    with options(**OLD):
        for name, mask in masks_for(zero, 23):
            for bname, lo, shift, nbins, H in hist_binnings(w, D):
                want = hm.histogram_rows(data, chunk_len, D, mask, lo, shift, nbins, H)
                for fam, cpg, family in legs(w, D, "histogram"):
                    no_fast(fam)
                    chunks_per_group(cpg)
                    with ran(only=[family], **{family: 1}):
                        check_hist(data, batch, codec, w // 8, D, chunk_len, mask, lo, shift, nbins, H, (codec, w, D, kind, name, bname, family, cpg), want)


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_groupby_rows_over_runs(sz, oracle, no_fast, chunks_per_group, codec, w, D, kind):
    cd, batch, data, chunk_len, zero = rowop_batch(sz, oracle, codec, w, D, kind)
    key = GBY_KEY[(w, D)]
    key_lo, shift, nbins = gby_binning(w)
    with options(**OLD):
        for name, mask in masks_for(zero, 24):
            for H in GBY_TABLES:
                want = gbm.groupby_rows(data, chunk_len, D, key, mask, key_lo, shift, nbins, H)
                for fam, cpg, family in legs(w, D, "groupby"):
                    no_fast(fam)
                    chunks_per_group(cpg)
                    with ran(only=[family], **{family: 1}):
                        check_gby(data, batch, codec, w // 8, D, chunk_len, key, mask, key_lo, shift, nbins, H, (codec, w, D, kind, name, H, family, cpg), want)


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_filter_linear_over_runs(sz, oracle, no_fast, chunks_per_group, codec, w, D, kind):
    """mask and counts of a sum, a change (through filter_change) and a lag term with w + u != 0; then both lag terms once more through
    the C entry point with a NULL mask, counts alone, and a scratch filled with one sentinel and with another: the seam pass has the
    chunks' first[] and last[] rows alone to go by"""
    import torch
    cd, batch, data, chunk_len, _ = rowop_batch(sz, oracle, codec, w, D, kind)
    col = LIN_COL[(w, D)]
    with options(**OLD):
        for name, wt, u, bias, lo, hi in linear_sets(data, D, col):
            want = lm.filter_linear(data, chunk_len, D, wt, lo, hi, u, bias)
            for fam, cpg, family in legs(w, D, "linear"):
                no_fast(fam)
                chunks_per_group(cpg)
                with ran(only=[family], **{family: 1}):               # one decode launch; the seam pass is no kernel family
                    if name == "change":
                        got = cd.filter_change(batch, col, lo=lo, hi=hi)
                        mask, counts = got["mask"].cpu().numpy(), got["counts"].cpu().numpy().astype(np.int64)
                    else:
                        mask, counts = run_linear(cd, batch, wt, lo, hi, u, bias)
                msg = (codec, w, D, kind, name, family, cpg)
                assert np.array_equal(counts, want[1]), ("counts",) + msg + (counts.tolist(), want[1].tolist())
                assert np.array_equal(mask, want[0]), ("mask",) + msg + ("first wrong (chunk, byte)", tuple(np.argwhere(mask != want[0])[0]))
                for sent in ((0x5A, 0xA5) if u is not None else ()):   # (whatever the scratch held: a first[] the decode did not store shows)
                    tmp = torch.full((sz._lib.filter_linear_tmp_bytes(w // 8, NCHUNKS, D),), sent, dtype=torch.uint8, device="cuda")
                    k = torch.full((NCHUNKS + 8,), -77, dtype=torch.int32, device="cuda")
                    with ran(only=[family], **{family: 1}):
                        raw_linear(sz, cd, batch, codec, w // 8, D, chunk_len, wt, u, bias, lo, hi, None, k, None, tmp)
                    k = k.cpu().numpy()
                    assert np.array_equal(k[:NCHUNKS], want[1]) and np.all(k[NCHUNKS:] == -77), ("counts, NULL mask", sent) + msg + (k.tolist(), want[1].tolist())


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_zone_map_and_pruning_over_runs(sz, oracle, no_fast, chunks_per_group, codec, w, D, kind):
    """the map against the raw samples; then filter_rows and filter_linear on one band with zones=: bit for bit the unpruned call's
    result and the model's.  (Where zone_band finds no band -- FIRE at 8 bits sweeps every column over the whole range in every
    chunk -- the band is column 0's upper half: every chunk must be decoded, and the zoned call is the plain one.)"""
    cd, batch, data, chunk_len, _ = rowop_batch(sz, oracle, codec, w, D, kind)
    band = zone_band(data, chunk_len, D, w)
    prunes = band is not None
    (lo, hi), (wt, llo, lhi) = band_bounds(band if prunes else (0, 1 << (w - 1)), w, D)
    zone = zm.zone_map(data, chunk_len, D, w // 8)
    cls = zm.classify_box(*zone, lo, hi, fm.ALL, D)
    assert np.array_equal(cls, zm.classify_linear(*zone, wt, 0, llo, lhi, D))
    want = fm.filter_rows(data, chunk_len, D, lo, hi, fm.ALL)
    wlin = lm.filter_linear(data, chunk_len, D, wt, llo, lhi)
    assert np.array_equal(want[0], wlin[0])
    with options(**OLD):
        for fam, cpg, family in legs(w, D, "window"):
            no_fast(fam)
            chunks_per_group(cpg)
            msg = (codec, w, D, kind, family, cpg)
            with ran(only=[family], **{family: 1}):                   # the map is the windowed query with one window a chunk
                z = cd.zone_map(batch)
            assert_zone_map(z, data, chunk_len, D, w // 8, msg)
            survivors = int((cls == zm.DECODE).sum())
            for name, call in (("filter_rows", lambda zones: cd.filter_rows(batch, list(map(int, lo)), list(map(int, hi)), zones=zones)),
                               ("filter_linear", lambda zones: cd.filter_linear(batch, [int(v) for v in wt], lo=llo, hi=lhi, zones=zones))):
                with ran(only=[family], **{family: 1}):
                    plain = call(None)
                cd.last_prune = None
                with ran(only=[family], **{family: 1}):
                    got = call(z)
                for which, g in (("unpruned", plain), ("zones", got)):
                    assert np.array_equal(g["counts"].cpu().numpy().astype(np.int64), want[1]), (name, which, "counts") + msg
                    assert np.array_equal(g["mask"].cpu().numpy(), want[0]), (name, which, "mask") + msg
                lp = cd.last_prune
                assert lp["survivors"] == survivors and np.array_equal(lp["class"].cpu().numpy(), cls), (name, "classes") + msg
                assert (2 <= survivors <= NCHUNKS - 2) if prunes else survivors == NCHUNKS, (name, survivors) + msg


# ------------------------------------------------------------------ a chunk rejected at its header in the middle of a lane group


def keep_chunks():
    return np.arange(NCHUNKS) != BAD


def assert_rets(r, chunk_len, msg):
    assert r[BAD] < 0 and np.all(r[keep_chunks()] == chunk_len), ("rets",) + msg + (r.tolist(),)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_damaged_chunk_in_a_group_query_windows(sz, damaged, codec, w, D):
    import torch
    cd, batch, data, chunk_len, _ = damaged(codec, w, D)
    W = 24
    want = wm.chunk_windows(data, chunk_len, D, W)
    with ran(only=["dec_fast"], dec_fast=2):
        res = cd.query_windows(batch, W, per_chunk=True, check=False)
        rets = torch.full((NCHUNKS + 1,), -77, dtype=torch.int64, device="cuda")
        sz._lib.check(sz._lib.query_windows(sz._lib.CODEC_DELTA if codec == "delta" else sz._lib.CODEC_XFF, w // 8, batch.data.data_ptr(),
                                            batch.offsets.data_ptr(), NCHUNKS, chunk_len, D, W, 7, 0, res["min"].data_ptr(), res["max"].data_ptr(),
                                            res["sum"].data_ptr(), rets.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    r = rets.cpu().numpy()
    assert r[NCHUNKS] == -77
    assert_rets(r[:NCHUNKS], chunk_len, (codec, w, D))
    keep = keep_chunks()
    for k, wv in zip(("min", "max", "sum"), want):
        g = res[k].cpu().numpy()
        g = g.view(np.uint64) if k == "sum" else g
        assert np.array_equal(g[keep].astype(np.uint64), wv[keep].astype(np.uint64)), (k, codec, w, D)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_damaged_chunk_in_a_group_zone_map(sz, damaged, codec, w, D):
    from rowop_runners import host
    cd, batch, data, chunk_len, _ = damaged(codec, w, D)
    zmin, zmax, zlen = zm.zone_map(data, chunk_len, D, w // 8)
    with ran(only=["dec_fast"], dec_fast=1):
        z = cd.zone_map(batch)
    keep = keep_chunks()
    assert_rets(host(z.len), chunk_len, (codec, w, D))
    assert np.array_equal(host(z.min)[keep], zmin[keep]) and np.array_equal(host(z.max)[keep], zmax[keep]), (codec, w, D)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_damaged_chunk_in_a_group_filter_rows(sz, damaged, codec, w, D):
    import torch
    cd, batch, data, chunk_len, _ = damaged(codec, w, D)
    name, mode, lo, hi, _ = bound_sets(data, chunk_len, w // 8, D)[0][0]
    want = fm.filter_rows(data, chunk_len, D, lo, hi, mode)
    MB = fm.geometry(chunk_len, D)[1]
    dt = torch.uint8 if w == 8 else torch.uint16
    lo_t, hi_t = (torch.from_numpy(v.astype(np.int32)).cuda().to(dt) for v in (lo, hi))
    mask = torch.full((NCHUNKS * MB + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    counts = torch.full((NCHUNKS + 8,), -77, dtype=torch.int32, device="cuda")
    rets = torch.full((NCHUNKS,), -77, dtype=torch.int64, device="cuda")
    with ran(only=["dec_fast"], dec_fast=1):
        sz._lib.check(sz._lib.filter_rows(sz._lib.CODEC_DELTA if codec == "delta" else sz._lib.CODEC_XFF, w // 8, batch.data.data_ptr(),
                                          batch.offsets.data_ptr(), NCHUNKS, chunk_len, D, lo_t.data_ptr(), hi_t.data_ptr(), mode, 0, mask.data_ptr(),
                                          counts.data_ptr(), rets.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert_rets(rets.cpu().numpy(), chunk_len, (codec, w, D))
    keep = keep_chunks()
    m, k = mask.cpu().numpy(), counts.cpu().numpy()
    assert np.all(m[NCHUNKS * MB:] == 0x5A) and np.all(k[NCHUNKS:] == -77)
    assert np.array_equal(m[:NCHUNKS * MB].reshape(NCHUNKS, MB)[keep], want[0][keep]) and np.array_equal(k[:NCHUNKS][keep], want[1][keep]), (codec, w, D)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_damaged_chunk_in_a_group_select_rows(sz, damaged, codec, w, D):
    cd, batch, data, chunk_len, mask = damaged(codec, w, D)
    cnt = sm.counts(mask, data.size, chunk_len, D)
    total = int(cnt.sum())
    bases = sm.prefix_bases(cnt)
    elem, ident = sentinels(w // 8, 0x5A)
    want_rows, want_ids = sm.select_rows(data, chunk_len, D, mask, bases, total, sentinel=elem, id_sentinel=ident)
    with ran(only=["dec_fast"], dec_fast=1):
        rows, ids, rets = run_select(batch, codec, w // 8, D, chunk_len, mask, bases, total, total)
    assert_rets(rets, chunk_len, (codec, w, D))
    keep = np.ones(total, bool)
    keep[int(bases[BAD]):int(bases[BAD] + cnt[BAD])] = False           # the damaged chunk's span alone is unspecified
    assert np.all(rows[total * D:] == elem) and np.all(ids[total:] == ident)
    assert np.array_equal(rows[:total * D].reshape(total, D)[keep], want_rows[keep]) and np.array_equal(ids[:total][keep], want_ids[keep]), (codec, w, D)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_damaged_chunk_in_a_group_aggregate_rows(sz, damaged, codec, w, D):
    cd, batch, data, chunk_len, mask = damaged(codec, w, D)
    for W in WINDOWS:                                      # (the operation takes no NULL mask)
        with ran(only=["dec_fast"], dec_fast=1):
            check_agg(data, batch, codec, w // 8, D, chunk_len, mask, W, (codec, w, D, W), skip_chunk=BAD)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_damaged_chunk_in_a_group_extrema_rows(sz, damaged, codec, w, D):
    cd, batch, data, chunk_len, mask = damaged(codec, w, D)
    for m in (mask, None):
        with ran(only=["dec_fast"], dec_fast=1):
            check_ext(data, batch, codec, w // 8, D, chunk_len, m, 24, (codec, w, D, m is None), skip_chunk=BAD)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_damaged_chunk_in_a_group_moments_rows(sz, damaged, codec, w, D):
    cd, batch, data, chunk_len, mask = damaged(codec, w, D)
    for m in (mask, None):
        with ran(only=["dec_fast"], dec_fast=1):
            check_mom(data, batch, codec, w // 8, D, chunk_len, m, 24, D - 1, (codec, w, D, m is None), skip_chunk=BAD)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_damaged_chunk_in_a_group_histogram_rows(sz, damaged, codec, w, D):
    """a histogram a chunk: the damaged chunk's alone is unspecified"""
    cd, batch, data, chunk_len, mask = damaged(codec, w, D)
    bname, lo, shift, nbins, _ = hist_binnings(w, D)[0]
    for m in (mask, None):
        with ran(only=["dec_fast"], dec_fast=1):
            check_hist(data, batch, codec, w // 8, D, chunk_len, m, lo, shift, nbins, 1, (codec, w, D, m is None), skip_group=BAD, bad_chunk=BAD)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_damaged_chunk_in_a_group_groupby_rows(sz, damaged, codec, w, D):
    """a table a chunk: the damaged chunk's alone is unspecified"""
    cd, batch, data, chunk_len, mask = damaged(codec, w, D)
    key_lo, shift, nbins = gby_binning(w)
    for m in (mask, None):
        with ran(only=["dec_fast"], dec_fast=1):
            check_gby(data, batch, codec, w // 8, D, chunk_len, GBY_KEY[(w, D)], m, key_lo, shift, nbins, 1, (codec, w, D, m is None), skip_table=BAD, bad_chunk=BAD)


def damaged_linear(sz, damaged, codec, w, D, lag):
    """mask, counts and rets of the C entry point on sentinel-filled outputs and scratch.  Without a lag term every other chunk is the
    model's; with one, row 0 of the chunk behind the damage has lost its predecessor and is unspecified (as
    test_filter_linear_damaged_chunk has it), and every other row of that chunk and of the others is the model's"""
    import torch
    cd, batch, data, chunk_len, _ = damaged(codec, w, D)
    name, wt, u, bias, lo, hi = linear_sets(data, D, LIN_COL[(w, D)])[1 if lag else 0]
    assert (u is not None) == lag
    want = lm.filter_linear(data, chunk_len, D, wt, lo, hi, u, bias)
    MB = fm.geometry(chunk_len, D)[1]
    mask = torch.full((NCHUNKS * MB + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    counts = torch.full((NCHUNKS + 8,), -77, dtype=torch.int32, device="cuda")
    rets = torch.full((NCHUNKS,), -77, dtype=torch.int64, device="cuda")
    tmp = torch.full((sz._lib.filter_linear_tmp_bytes(w // 8, NCHUNKS, D),), 0x5A, dtype=torch.uint8, device="cuda") if lag else None
    with ran(only=["dec_fast"], dec_fast=1):
        raw_linear(sz, cd, batch, codec, w // 8, D, chunk_len, wt, u, bias, lo, hi, mask, counts, rets, tmp)
    assert_rets(rets.cpu().numpy(), chunk_len, (codec, w, D, lag))
    m, k = mask.cpu().numpy(), counts.cpu().numpy()
    assert np.all(m[NCHUNKS * MB:] == 0x5A) and np.all(k[NCHUNKS:] == -77)
    m = m[:NCHUNKS * MB].reshape(NCHUNKS, MB).copy()
    k = k[:NCHUNKS].astype(np.int64)
    if lag:
        bit = int(m[BAD + 1, 0] & 1), int(want[0][BAD + 1, 0] & 1)
        m[BAD + 1, 0] = (m[BAD + 1, 0] & 0xFE) | bit[1]
        k[BAD + 1] += bit[1] - bit[0]
    keep = keep_chunks()
    assert np.array_equal(k[keep], want[1][keep]), ("counts", codec, w, D, lag, k.tolist(), want[1].tolist())
    assert np.array_equal(m[keep], want[0][keep]), ("mask", codec, w, D, lag)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_damaged_chunk_in_a_group_filter_linear(sz, damaged, codec, w, D):
    damaged_linear(sz, damaged, codec, w, D, False)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_damaged_chunk_in_a_group_filter_change(sz, damaged, codec, w, D):
    damaged_linear(sz, damaged, codec, w, D, True)


# ------------------------------------------------------------------ ... and a chunk that goes wrong at its END in the middle of a group


TRUNCATED_WINDOW = 64                                  # 32 windows a chunk: the last one takes blocks 248 .. 255, of which 255 is the verbatim tail's


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_truncated_chunk_in_a_group_extrema_rows(sz, truncated, codec, w, D):
    cd, batch, data, chunk_len, mask = truncated(codec, w, D)
    for m in (None, mask):
        with ran(only=["dec_fast"], dec_fast=1):
            check_ext(data, batch, codec, w // 8, D, chunk_len, m, TRUNCATED_WINDOW, (codec, w, D, m is None), skip_chunk=BAD)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_truncated_chunk_in_a_group_moments_rows(sz, truncated, codec, w, D):
    cd, batch, data, chunk_len, mask = truncated(codec, w, D)
    for m in (None, mask):
        with ran(only=["dec_fast"], dec_fast=1):
            check_mom(data, batch, codec, w // 8, D, chunk_len, m, TRUNCATED_WINDOW, 0, (codec, w, D, m is None), skip_chunk=BAD)


@pytest.mark.parametrize("codec,w,D", DAMAGE_SHAPES, ids=DAMAGE_IDS)
def test_truncated_chunk_in_a_group_aggregate_rows(sz, truncated, codec, w, D):
    cd, batch, data, chunk_len, mask = truncated(codec, w, D)
    with ran(only=["dec_fast"], dec_fast=1):
        check_agg(data, batch, codec, w // 8, D, chunk_len, mask, TRUNCATED_WINDOW, (codec, w, D), skip_chunk=BAD)


# ------------------------------------------------------------------ 3. the FIRE counter drive

FIRE_KEY = 1                                           # group-by: the key column (8 columns only)


@pytest.mark.parametrize("w,D", list(FIRE_SHAPES), ids=FIRE_IDS)
def test_extrema_rows_on_the_fire_drive(sz, oracle, chunks_per_group, w, D):
    cd, batch, data, chunk_len, nchunks = fire_batch(sz, oracle, w, D)
    R = chunk_len // D
    cases = [(batch, data, name, mask) for name, mask in (("none", None), ("3 of 8", three_of_8(nchunks, R)))]
    px, pmask = fire_patched(w, D)
    cases.append((fire_batch(sz, oracle, w, D, px)[1], px, "all ones and 0 alone in their windows", pmask))
    for b, x, name, mask in cases:
        for W in fire_windows(w, D):
            want = em.extrema_rows(x, chunk_len, D, mask, W)
            for family, cpg in fire_legs(sz, w, D, chunks_per_group):
                with ran(only=[family], **{family: 1}):
                    check_ext(x, b, "xff", w // 8, D, chunk_len, mask, W, (w, D, name, W, family, cpg), want, ops=255)


@pytest.mark.parametrize("w,D", list(FIRE_SHAPES), ids=FIRE_IDS)
def test_moments_rows_on_the_fire_drive(sz, oracle, chunks_per_group, w, D):
    cd, batch, data, chunk_len, nchunks = fire_batch(sz, oracle, w, D)
    for name, mask in (("none", None), ("3 of 8", three_of_8(nchunks, chunk_len // D))):
        for W in fire_windows(w, D):
            want = mm.moments_rows(data, chunk_len, D, mask, W, 0)
            for family, cpg in fire_legs(sz, w, D, chunks_per_group):
                with ran(only=[family], **{family: 1}):
                    check_mom(data, batch, "xff", w // 8, D, chunk_len, mask, W, 0, (w, D, name, W, family, cpg), want)


@pytest.mark.parametrize("w,D", list(FIRE_SHAPES), ids=FIRE_IDS)
def test_histogram_rows_on_the_fire_drive(sz, oracle, chunks_per_group, w, D):
    """256 bins over the whole range, one histogram a batch and one a chunk"""
    cd, batch, data, chunk_len, nchunks = fire_batch(sz, oracle, w, D)
    for name, mask in (("none", None), ("3 of 8", three_of_8(nchunks, chunk_len // D))):
        for H in (0, 1):
            want = hm.histogram_rows(data, chunk_len, D, mask, None, w - 8, 256, H)
            for family, cpg in fire_legs(sz, w, D, chunks_per_group):
                with ran(only=[family], **{family: 1}):
                    check_hist(data, batch, "xff", w // 8, D, chunk_len, mask, None, w - 8, 256, H, (w, D, name, H, family, cpg), want)


def test_groupby_rows_on_the_fire_drive(sz, oracle, chunks_per_group):
    w, D = 8, 8
    cd, batch, data, chunk_len, nchunks = fire_batch(sz, oracle, w, D)
    for name, mask in (("none", None), ("3 of 8", three_of_8(nchunks, chunk_len // D))):
        for H in (0, 1):
            want = gbm.groupby_rows(data, chunk_len, D, FIRE_KEY, mask, 0, 0, 256, H)
            for family, cpg in fire_legs(sz, w, D, chunks_per_group):
                with ran(only=[family], **{family: 1}):
                    check_gby(data, batch, "xff", w // 8, D, chunk_len, FIRE_KEY, mask, 0, 0, 256, H, (w, D, name, H, family, cpg), want)


@pytest.mark.parametrize("w,D", list(FIRE_SHAPES), ids=FIRE_IDS)
def test_filter_change_on_the_fire_drive(sz, oracle, chunks_per_group, w, D):
    cd, batch, data, chunk_len, nchunks = fire_batch(sz, oracle, w, D)
    lo, hi = fire_change_bounds(data, D)
    want = lm.filter_change(data, chunk_len, D, FIRE_COL, lo, hi)
    for family, cpg in fire_legs(sz, w, D, chunks_per_group):
        with ran(only=[family], **{family: 1}):
            got = cd.filter_change(batch, FIRE_COL, lo=lo, hi=hi)
        counts = got["counts"].cpu().numpy().astype(np.int64)
        assert np.array_equal(counts, want[1]), ("counts", w, D, family, cpg, counts.tolist(), want[1].tolist())
        assert np.array_equal(got["mask"].cpu().numpy(), want[0]), ("mask", w, D, family, cpg)
