"""CPU tier of tests/test_gpu_rowop_drive.py: the drives must GET THERE.  On the models and the schedules alone, without a device: the
batches, masks, binnings, predicates and bands of the GPU tier reach the edges they are there for -- a batch that stops reaching one
fails here and not silently --, each model equals a one-row-at-a-time restatement in Python integers on a small drive batch, and the GPU
tier's kernel-family literals are what the planner plans, at one and at three chunks a lane group."""
import numpy as np
import pytest

import extrema_model as em
import filter_model as fm
import fire_drive as fd
import groupby_model as gbm
import histogram_model as hm
import linear_model as lm
import moments_model as mm
import planner
import rle_drive as rd
import zone_model as zm
from drive_tables import (CPGS, DAMAGE_SHAPES, FIRE_COL, FIRE_SHAPES, GBY_KEY, GBY_TABLES, LIN_COL, NB, NCHUNKS,
                          PATCH_CHUNK, PATCH_TOP, PATCH_ZERO, ROWOP_KINDS, ROWOP_SHAPES, WINDOWS, band_bounds, batch_of, fire_change_bounds,
                          fire_patched, fire_rows, fire_windows, gby_binning, hist_binnings, linear_sets, masks_for, refs_for, three_of_8, zone_band)
from planner import CODEC, QUERY, plan_shape, probe  # noqa: F401  (fixtures)
from rowdata import bound_sets
from streams import OLD, fire_batch_of

R = 8 * NB
SHAPES = list(ROWOP_SHAPES)
KINDS = ROWOP_KINDS
W24 = 24                                               # windows of 3 blocks
assert KINDS == ("lengths", "start", "alternate", "tails") and WINDOWS == (8, W24) and SHAPES == [(16, 8), (8, 32), (16, 12)]


def runs_of(z):
    """[(first block, one past the last)] of a chunk's runs"""
    edges = np.flatnonzero(np.diff(np.concatenate([[0], z.astype(np.int8), [0]])))
    return list(zip(edges[::2].tolist(), edges[1::2].tolist()))


def batch(codec, w, D, kind):
    return batch_of(codec, w, D, kind, NCHUNKS, NB)


def test_runs_against_windows_of_three_blocks():
    """over the four kinds there is a window that a run enters, one that a run leaves, one wholly inside a run, and one that holds a
    whole run of one block between two packed blocks"""
    seen = set()
    for kind in KINDS:
        for z in rd.schedules(kind, NCHUNKS, NB):
            for a, b in runs_of(z):
                first, last = a // 3, (b - 1) // 3             # the windows of the run's first and last block
                if first != last:
                    seen.add("enters" if a % 3 else "enters at the edge")
                    seen.add("leaves" if b % 3 else "leaves at the edge")
                if last - first >= 2:
                    seen.add("inside")
                if b - a == 1 and a % 3 == 1:
                    seen.add("one block between two packed ones")
    assert {"enters", "leaves", "inside", "one block between two packed ones"} <= seen, seen


@pytest.mark.parametrize("w,D", SHAPES)
@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_the_masks_select_what_they_are_there_for(codec, w, D):
    first_of_run = last_of_run = empty = False
    for kind in KINDS:
        data, chunk_len, zero = batch(codec, w, D, kind)
        masks = dict(masks_for(zero, 21))
        out = em.extrema_rows(data, chunk_len, D, masks["outside runs"], W24)
        empty |= bool(np.any((out["count"] == 0) & np.all(out["rows"] == em.NO_ROW, axis=2) & np.all(out["argmin"] == em.NO_ROW, axis=2)))
        ins = em.extrema_rows(data, chunk_len, D, masks["inside runs"], W24)
        for c in range(NCHUNKS):
            rr = runs_of(zero[c])
            rows = ins["rows"][c][ins["count"][c] > 0]
            first_of_run |= bool(np.isin(rows[:, 0], [8 * a for a, _ in rr if a % 3]).any())           # (a run that starts inside its window)
            last_of_run |= bool(np.isin(rows[:, 1], [8 * b - 1 for _, b in rr if b % 3]).any())
        for name, mask in masks.items():                   # every mask selects some rows and not all
            n = int(em.selected(mask, data.size, chunk_len, D).sum())
            assert (0 < n < NCHUNKS * R) if mask is not None else n == NCHUNKS * R, (kind, name, n)
    assert empty and first_of_run and last_of_run, (empty, first_of_run, last_of_run)


@pytest.mark.parametrize("w,D", SHAPES)
def test_a_window_edge_cuts_a_run_at_its_extremum(w, D):
    """delta: some window's argmin or argmax is a row inside a run that is not the run's first row in the chunk but its first row in
    that window -- what run_selected_span's `f` must be when a run crosses a window edge"""
    hit = 0
    for kind in KINDS:
        data, chunk_len, zero = batch("delta", w, D, kind)
        for name, mask in masks_for(zero, 21):
            if name not in ("none", "inside runs"):
                continue
            want = em.extrema_rows(data, chunk_len, D, mask, W24)
            for c in range(NCHUNKS):
                cut = [win for a, b in runs_of(zero[c]) for win in range(a // 3 + 1, (b - 1) // 3 + 1)]      # windows a run enters from the one in front
                for win in cut:
                    hit += int((want["argmin"][c, win] == win * W24).sum() + (want["argmax"][c, win] == win * W24).sum())
    assert hit > 0


@pytest.mark.parametrize("w,D", SHAPES)
@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_start_opens_every_chunk_with_a_run(codec, w, D):
    data, chunk_len, zero = batch(codec, w, D, "start")
    assert zero[:, 0].all()
    col = LIN_COL[(w, D)]
    same = lm.filter_change(data, chunk_len, D, col, 0, 0)
    assert same[0][0, 0] & 1, "row 0 of chunk 0 is its own predecessor: no change"
    if codec == "delta":                                   # a delta chunk opens with zero rows, whatever the chunk in front ended with
        v = data.reshape(NCHUNKS, R, D)
        assert not v[:, :8].any()


@pytest.mark.parametrize("w,D", SHAPES)
@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_tails_end_in_runs_and_the_seams_have_work(oracle, codec, w, D):
    """A run slot never holds a chunk's LAST block: behind a run block the encoders go on only while two more blocks fit (`<`, and `<=`
    in the general FIRE layout), so a chunk that ends in zero blocks leaves at least its last block to the verbatim tail, remaining_len
    is never 0 behind a run, and the seam pass cannot be handed a chunk's last row by a run -- asserted here as what the format gives.
    What the "tails" batch does reach: streams whose LAST slot is a run, so that the tail's first row takes its predecessor from the run
    (lcarry); streams that end in two packed blocks with no tail at all (the last row comes from the last block); and seam rows whose
    predicate differs between the row as its own predecessor and the true one, so that the seam pass has something to put right"""
    data, chunk_len, zero = batch(codec, w, D, "tails")
    run_last = no_tail = 0
    for c, s in enumerate(oracle.compress_chunks(codec, data, chunk_len, D)):
        ngroups, remaining, slots = rd.slots(s, w, D)
        last = [sl for sl in slots if sl[2] != "pad"][-1]
        if last[2] == "run":
            assert remaining >= 8 * D and zero[c, NB - remaining // (8 * D) - 1], (c, remaining)
            run_last += 1
        no_tail += remaining == 0
        if zero[c, -1]:
            assert remaining >= 8 * D, (c, "a run reached the chunk's last block")
    assert run_last >= 2 and no_tail >= 1, (run_last, no_tail)
    seams = 0
    starts = range(0, NCHUNKS * R, R)
    for kind in KINDS:
        x, _, _ = batch(codec, w, D, kind)
        for name, wt, u, bias, lo, hi in linear_sets(x, D, LIN_COL[(w, D)]):
            if u is None:
                continue
            true = lm.filter_linear(x, chunk_len, D, wt, lo, hi, u, bias)[0]
            own = lm.filter_linear(x, chunk_len, D, wt, lo, hi, u, bias, self_rows=starts)[0]
            assert np.array_equal(true[:, 1:], own[:, 1:]) and np.array_equal(true[:, 0] & 0xFE, own[:, 0] & 0xFE)
            seams += int(((true[:, 0] ^ own[:, 0]) & 1).sum())
    assert seams >= 4, seams


@pytest.mark.parametrize("w,D", SHAPES)
def test_the_bins_take_some_runs_and_drop_others(w, D):
    key = GBY_KEY[(w, D)]
    data, chunk_len, zero = batch("delta", w, D, "lengths")
    v = data.reshape(NCHUNKS, R, D).astype(np.int64)
    moves = (v.max(axis=1) != v.min(axis=1)).sum(axis=0)
    assert key == next(d for d in range(1, D) if moves[d] >= 12) and moves[key] >= 12, moves.tolist()
    name, lo, shift, nbins, H = hist_binnings(w, D)[0]
    key_lo, kshift, knbins = gby_binning(w)
    assert name == "clip" and hist_binnings(w, D)[1][2] > 0
    for kind in KINDS:
        data, chunk_len, zero = batch("delta", w, D, kind)
        v = data.reshape(NCHUNKS, R, D).astype(np.int64)
        inside = np.zeros((NCHUNKS, D), bool)                # a run's value of column d lies inside the bins in chunk c / outside
        outside = np.zeros((NCHUNKS, D), bool)
        kin = kout = 0
        for c in range(NCHUNKS):
            for a, b in runs_of(zero[c]):
                row = v[c, 8 * a]
                ok = (((row - lo) % (1 << w)) >> shift) < nbins
                inside[c] |= ok
                outside[c] |= ~ok
                k_ok = (((row[key] - key_lo) % (1 << w)) >> kshift) < knbins
                kin += k_ok
                kout += not k_ok
        only_out = outside & ~inside
        assert (inside.any(axis=0) & only_out.any(axis=0)).any(), kind       # a column whose runs are all dropped in one chunk, and counted in another
        assert kin > 0 and kout > 0, (kind, kin, kout)
        hist = hm.histogram_rows(data, chunk_len, D, None, lo, shift, nbins, 0)
        assert 0 < int(hist.sum()) < data.size


@pytest.mark.parametrize("w,D", SHAPES)
@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_every_predicate_splits_the_rows(codec, w, D):
    for kind in KINDS:
        data, chunk_len, zero = batch(codec, w, D, kind)
        for name, wt, u, bias, lo, hi in linear_sets(data, D, LIN_COL[(w, D)]):
            n = int(lm.filter_linear(data, chunk_len, D, wt, lo, hi, u, bias)[1].sum())
            assert 0 < n < NCHUNKS * R, (kind, name, n)
        if kind == "lengths":                              # the damaged-chunk cases' box filter
            name, mode, lo, hi, _ = bound_sets(data, chunk_len, w // 8, D)[0][0]
            assert 0 < int(fm.filter_rows(data, chunk_len, D, lo, hi, mode)[1].sum()) < NCHUNKS * R


@pytest.mark.parametrize("w,D", SHAPES)
@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_the_zone_band_prunes_and_keeps(codec, w, D):
    """at least two chunks decided by the map and at least two left to the decoder -- except under FIRE at 8 bits, where the drive sweeps
    every column over the whole range in every chunk and NO box can decide a chunk: there the band keeps all sixteen"""
    for kind in KINDS:
        data, chunk_len, _ = batch(codec, w, D, kind)
        band = zone_band(data, chunk_len, D, w)
        zone = zm.zone_map(data, chunk_len, D, w // 8)
        if (codec, w) == ("xff", 8):
            span = zone[1].astype(np.int64) - zone[0].astype(np.int64)
            assert band is None and int((span < 254).sum()) == 0 and int((span.min(axis=1) < 255).sum()) <= 1, kind
            band = (0, 1 << (w - 1))
        (lo, hi), (wt, llo, lhi) = band_bounds(band, w, D)
        cls = zm.classify_box(*zone, lo, hi, fm.ALL, D)
        assert np.array_equal(cls, zm.classify_linear(*zone, wt, 0, llo, lhi, D))
        survivors = int((cls == zm.DECODE).sum())
        assert (survivors == NCHUNKS) if (codec, w) == ("xff", 8) else (2 <= survivors <= NCHUNKS - 2), (kind, band, cls.tolist())
        n = int(fm.filter_rows(data, chunk_len, D, lo, hi, fm.ALL)[1].sum())
        assert 0 < n < NCHUNKS * R, (kind, n)


@pytest.mark.parametrize("w,D", list(FIRE_SHAPES))
def test_the_fire_cases_select_and_reach_the_identities(w, D):
    nchunks = FIRE_SHAPES[(w, D)][0]
    data, chunk_len = fire_batch_of(w, D, nchunks)
    rows = fire_rows(w, D)
    assert chunk_len == rows * D and fire_windows(w, D) == (64, rows) and rows % 64 == 0
    assert (w, D, nchunks, rows) in ((8, 8, 7, 8 * fd.NB8), (16, 1, 5, 8 * fd.NB16))
    lo, hi = fire_change_bounds(data, D)
    assert 0 < int(lm.filter_change(data, chunk_len, D, FIRE_COL, lo, hi)[1].sum()) < nchunks * rows
    m38 = three_of_8(nchunks, rows)
    assert int(em.selected(m38, data.size, chunk_len, D).sum()) == 3 * nchunks * rows // 8
    # the edges behind the extrema identities: a selected all-ones value is a minimum with a row, a selected 0 a maximum with a row
    top = (1 << w) - 1
    px, pmask = fire_patched(w, D)
    assert 0 < int(em.selected(pmask, px.size, chunk_len, D).sum()) < nchunks * rows
    want = em.extrema_rows(px, chunk_len, D, pmask, 64)
    wt, wz = PATCH_TOP // 64, PATCH_ZERO // 64
    assert PATCH_CHUNK < nchunks and wt != wz
    assert np.all(want["min"][PATCH_CHUNK, wt] == top) and np.all(want["argmin"][PATCH_CHUNK, wt] == PATCH_TOP) and want["count"][PATCH_CHUNK, wt] == 1
    assert np.all(want["max"][PATCH_CHUNK, wz] == 0) and np.all(want["argmax"][PATCH_CHUNK, wz] == PATCH_ZERO) and want["count"][PATCH_CHUNK, wz] == 1
    # (the drive itself sweeps the element range in every chunk, to within 1 %, but leaves no window to one value: hence the two rows)
    v = data.reshape(nchunks, rows, D).astype(np.int64)
    assert np.all(v.max(axis=1) - v.min(axis=1) >= top - top // 100)
    plain = em.extrema_rows(data, chunk_len, D, m38, 64)
    assert not np.any((plain["min"] == top) & (plain["count"][..., None] > 0)) and not np.any((plain["max"] == 0) & (plain["count"][..., None] > 0))


# ------------------------------------------------------------------ each model against a one-row-at-a-time restatement in Python integers

def zone_map_brute(x, chunk_len, D, w):
    top = (1 << w) - 1
    n = -(-len(x) // chunk_len)
    zmin, zmax, zlen = [[top] * D for _ in range(n)], [[0] * D for _ in range(n)], [0] * n
    for i, e in enumerate(int(v) for v in x):
        c, d = i // chunk_len, (i % chunk_len) % D
        zmin[c][d], zmax[c][d] = min(zmin[c][d], e), max(zmax[c][d], e)
        zlen[c] += 1
    return zmin, zmax, zlen


def classes_brute(x, chunk_len, D, match):
    """what a chunk's class must be CONSISTENT with, from the rows themselves: NONE only if no row matches, ALL only if every row does"""
    Rr = chunk_len // D
    rows = [[int(v) for v in x[i * D:(i + 1) * D]] for i in range(len(x) // D)]
    out = []
    for c in range(-(-len(rows) // Rr)):
        hits = [match(r) for r in rows[c * Rr:(c + 1) * Rr]]
        out.append({zm.DECODE} | ({zm.NONE} if not any(hits) else set()) | ({zm.ALL} if all(hits) else set()))
    return out


def filter_rows_brute(x, chunk_len, D, lo, hi, mode):
    Rr, MB = fm.geometry(chunk_len, D)
    n = -(-len(x) // chunk_len)
    mask, counts = np.zeros((n, MB), np.uint8), np.zeros(n, np.int64)
    for gr in range(len(x) // D):
        hits = [int(lo[d]) <= int(x[gr * D + d]) <= int(hi[d]) for d in range(D)]
        if all(hits) if mode == fm.ALL else any(hits):
            c, r = divmod(gr, Rr)
            mask[c, r >> 3] |= 1 << (r & 7)
            counts[c] += 1
    return mask, counts


@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_the_models_against_brute_force(codec):
    """uint8 x 5, 2 chunks of 48 blocks of the "lengths" drive"""
    w, D = 8, 5
    x, chunk_len, zero = rd.batch(codec, w, D, "lengths", 2, 48)
    masks = masks_for(zero, 5)
    for name, mask in masks:
        for W in WINDOWS:
            a, b = em.extrema_rows(x, chunk_len, D, mask, W), em.extrema_rows_brute(x, chunk_len, D, mask, W)
            assert all(np.array_equal(a[k], b[k]) for k in a), ("extrema", name, W)
            for ref in refs_for(D):
                a, b = mm.moments_rows(x, chunk_len, D, mask, W, ref), mm.moments_rows_brute(x, chunk_len, D, mask, W, ref)
                assert all(np.array_equal(a[k].astype(np.uint64), np.array(b[k], np.uint64)) for k in a), ("moments", name, W, ref)
        for bname, lo, shift, nbins, H in hist_binnings(w, D):
            assert np.array_equal(hm.histogram_rows(x, chunk_len, D, mask, lo, shift, nbins, H), hm.histogram_rows_brute(x, chunk_len, D, mask, lo, shift, nbins, H)), (name, bname)
        key_lo, shift, nbins = gby_binning(w)
        for H in GBY_TABLES:
            a, b = gbm.groupby_rows(x, chunk_len, D, 1, mask, key_lo, shift, nbins, H), gbm.groupby_rows_brute(x, chunk_len, D, 1, mask, key_lo, shift, nbins, H)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), ("groupby", name, H)
    for name, wt, u, bias, lo, hi in linear_sets(x, D, 1):
        a, b = lm.filter_linear(x, chunk_len, D, wt, lo, hi, u, bias), lm.filter_linear_brute(x, chunk_len, D, wt, lo, hi, u, bias)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and 0 < int(a[1].sum()) < x.size // D, ("linear", name)
    zmin, zmax, zlen = zm.zone_map(x, chunk_len, D, w // 8)
    bmin, bmax, blen = zone_map_brute(x, chunk_len, D, w)
    assert zmin.tolist() == bmin and zmax.tolist() == bmax and zlen.tolist() == blen
    for d in range(D):
        for thr in (1, 64, 128, 255):
            (lo, hi), (wt, llo, lhi) = band_bounds((d, thr), w, D)
            cls = zm.classify_box(zmin, zmax, zlen, lo, hi, fm.ALL, D)
            assert np.array_equal(cls, zm.classify_linear(zmin, zmax, zlen, wt, 0, llo, lhi, D))
            assert all(int(k) in ok for k, ok in zip(cls, classes_brute(x, chunk_len, D, lambda r: r[d] >= thr))), (d, thr)     # noqa: B023
            a, b = fm.filter_rows(x, chunk_len, D, lo, hi, fm.ALL), filter_rows_brute(x, chunk_len, D, lo, hi, fm.ALL)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (d, thr)
            assert np.array_equal(a[0], lm.filter_linear(x, chunk_len, D, wt, llo, lhi)[0])


# ------------------------------------------------------------------ the GPU tier's kernel-family literals, replayed through the planner

LATER_OPS = ("histogram", "moments", "groupby", "extrema", "linear")


def plan(**fields):
    """-> (family, {every other field of the plan})"""
    return planner.split(planner.ask("decode", **fields))


def table_wg_chunks(wg_chunks, chunk_len, D, row_max):
    """plan.h: a workgroup's table of uint32 takes at most row_max a row of its chunks"""
    return wg_chunks if wg_chunks * (chunk_len // D) * row_max <= 0xFFFFFFFF else 0


def lanes(D):
    dp = 4
    while dp < D and dp < 64:
        dp <<= 1
    return dp


def test_the_gpu_tiers_literals_are_the_planners(probe):
    """every family tests/test_gpu_rowop_drive.py asserts from the dispatch counters is what csrc/plan.h plans for that shape, NO_FAST
    0 and 1, one and three chunks a lane group -- with the largest table of each case; and at three chunks a group a workgroup adds up
    three times the chunks in its table, or none where their rows could wrap an entry"""
    for (w, D), want in ROWOP_SHAPES.items():
        esz, chunk_len = w // 8, 8 * NB * D
        for codec in ("delta", "xff"):
            for no_fast in (0, 1):
                for cpg in CPGS:
                    kw = dict(esz=esz, D=D, chunk_len=chunk_len, nchunks=NCHUNKS, codec=CODEC[codec], no_fast=no_fast, chunks_per_group=cpg)
                    msg = (w, D, codec, no_fast, cpg)
                    shape = dict(plan_shape(codec, w, D, chunk_len, NCHUNKS, no_fast=no_fast, **OLD), chunks_per_group=cpg)
                    for op in ("moments", "window", "filter", "aggregate", "select"):
                        got, = probe(("decode", dict(shape, q=QUERY[op])))
                        assert got.get("family") == ("dec_generic" if no_fast else want[op]), (op,) + msg + (got,)
                        if got.get("family") == "dec_fast":
                            assert got["chunks_per_group"] == cpg
                    assert plan(q=QUERY["extrema"], **kw)[0] == ("dec_generic" if no_fast else want["extrema"]), msg
                    assert plan(q=QUERY["linear"], **kw)[0] == ("dec_generic" if no_fast else want["linear"]), msg
                    tables = [("histogram", D * max(b[3] for b in hist_binnings(w, D)), 1), ("groupby", gby_binning(w)[2] * (D + 1), (1 << w) - 1)]
                    for op, entries, row_max in tables:
                        fam, f = plan(q=QUERY[op], table_entries=entries, table_row_max=row_max, **kw)
                        assert fam == ("dec_generic" if no_fast else want[op]), (op,) + msg
                        per_wg = 256 // lanes(D) * (cpg if fam == "dec_fast" else 1)
                        assert f["wg_chunks"] == table_wg_chunks(per_wg, chunk_len, D, row_max), (op,) + msg + (f,)
                        assert f["lds"] <= 80 * 1024 and (f["table_off"] > 0) == (fam == "dec_fast")
    # the group-by sums of uint16 x 8 sit on the rule's edge: 32 chunks of 2 048 rows fit an entry, 96 do not
    assert table_wg_chunks(32, 8 * NB * 8, 8, 65535) == 32 and table_wg_chunks(96, 8 * NB * 8, 8, 65535) == 0
    assert DAMAGE_SHAPES == [(c, w, D) for c in ("delta", "xff") for (w, D) in ((16, 8), (8, 32))]       # (dec_fast for every mode, select rows included)
    assert all(ROWOP_SHAPES[(w, D)][op] == "dec_fast" for _, w, D in DAMAGE_SHAPES for op in ("window", "filter", "select", "aggregate", *LATER_OPS))
    # the FIRE drive's shapes
    for (w, D), (nchunks, fire_legs) in FIRE_SHAPES.items():
        esz, chunk_len = w // 8, fire_rows(w, D) * D
        for opts, cpg, family in fire_legs:
            no_fast = opts.get("no_fast", 0)
            kw = dict(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=1, no_fast=no_fast, chunks_per_group=cpg)
            shape = dict(plan_shape("xff", w, D, chunk_len, nchunks, **dict(OLD, **opts)), chunks_per_group=cpg)
            got, = probe(("decode", dict(shape, q=QUERY["moments"])))
            assert got.get("family") == family, (w, D, opts, got)
            assert plan(q=QUERY["extrema"], **kw)[0] == family and plan(q=QUERY["linear"], **kw)[0] == family, (w, D, opts)
            assert plan(q=QUERY["histogram"], table_entries=D * 256, table_row_max=1, **kw)[0] == family, (w, D, opts)
            if D == 8:
                assert plan(q=QUERY["groupby"], table_entries=256 * (D + 1), table_row_max=255, **kw)[0] == family, (w, D, opts)
