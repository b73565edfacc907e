"""GPU tests (-m gpu): the RLE / group state machine driven through its edges on EVERY kernel that restates or walks it.

The encoders restate the machine by hand -- as five passes of wave scans over per-lane pieces of blocks (encode_blk.h's rle_walk_scan,
encode_lat.h), or sequentially (encode_wide.h, encode_fast.h, encode_uni.h, encode_kernel.h, any_ndims.hip) -- and every decoder and
row operation places its output through the runs it wrote.  The inputs are tests/rle_drive.py's five batches: run lengths 1 .. 16 and
126 .. 129 closing in both slots of a group, a packed block that opens a new group behind a run, zero / packed alternating, a run as
the stream's first slot, chunks that end in a run and 0 .. 3 packed blocks (the tail test, the padding slot) -- rotated by the chunk's
index, so that the edges sit on 16 consecutive block indices and the lanes of a wave that serve different chunks are in different states
(tests/test_rle_drive_cpu.py asserts that the batches get there) -- and the cap of 32 767 blocks.

Every case: compress -> the oracle's bytes and sizes for EVERY chunk -> decompress into a poisoned buffer -> the input, every return
value, nothing outside; then the ORACLE's container through the same decoder, so that an encoder and a decoder that are wrong in the same
way cannot agree with each other; and the kernel family on both sides from the dispatch counters (tests/dispatch.py), as literals that
tests/test_rle_drive_cpu.py replays through the planner without a device.  A batch's first chunk is the golden fixture's case
(tests/golden/golden_rledrive_v1, minted from the compiled reference by oracle/gen_golden_rledrive.py) where there is one.  Then the
row operations over the same batches, against the numpy models applied to the raw samples, at one and at three chunks a lane group of
decode_fast.h (SPRINTZ_OPT_CHUNKS_PER_GROUP); the later ones are in tests/test_gpu_rowop_drive.py.  Nothing here needs the reference."""
import json
import os
import zlib

import numpy as np
import pytest

import aggregate_model as am
import filter_model as fm
import gather_model as gm
import rle_drive as rd
import select_model as sm
import window_model as wm
from dispatch import ROUND6, ran
from harness import DTYPES
from drive_tables import (BOTH, CAP_CASES, CASES, LAT_SINGLE, NB, NCHUNKS, ROWOP_CASES, ROWOP_IDS, WINDOWS, batch_of, family_of, legs, oracle_batch,
                          rowop_batch, run_masks)
from fixtures import chunks_per_group, no_fast, sz  # noqa: F401  (fixtures)
from rowdata import bound_sets
from rowop_runners import check_agg, check_select, run_filter
from streams import DEF, DENSE, OLD, check_streams, options, to_device

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_rledrive_v1")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN + ".json") as f:
        manifest = json.load(f)["cases"]
    arrays = np.load(GOLDEN + ".npz")
    return {(m["codec"], m["w"], m["ndims"], m["kind"]): (m, arrays[m["name"]]) for m in manifest}


def decode_checked(cd, batch, data, chunk_len, nchunks, dec, fell, tag):
    """decompress into a poisoned buffer: the input, every return value, nothing outside"""
    import torch
    esz, n = data.dtype.itemsize, data.size
    obuf = torch.full((n + 16,), 0x5A, dtype=torch.int8 if esz == 1 else torch.int16, device="cuda:0").view(cd.dtype)
    rets = torch.full((nchunks + 1,), -77, dtype=torch.int64, device="cuda:0")
    with ran(only=[dec], never=ROUND6 if fell else (), what=tag, **{dec: 1}):
        cd.decompress_into(batch.data, batch.offsets, nchunks, obuf[:n], rets)
    r = rets.cpu().numpy()
    assert (r[:nchunks] == chunk_len).all() and r[nchunks] == -77, (tag, r)
    o = obuf.cpu().numpy().view(DTYPES[esz])
    bad = np.flatnonzero(o[:n] != data)
    assert bad.size == 0, (tag, "first wrong sample: chunk", int(bad[0]) // chunk_len, "block", (int(bad[0]) % chunk_len) // (8 * cd.ndims), "element", int(bad[0]) % chunk_len)
    assert (o[n:] == 0x5A).all(), (tag, "wrote outside the output")


def roundtrip_data(sz, oracle, codec, w, D, data, chunk_len, nchunks, enc, dec, tag, fixture=None):
    """fixture: (manifest entry, the compiled reference's stream) of the batch's first chunk"""
    (enc, enc_fell), (dec, dec_fell) = family_of(enc), family_of(dec)
    cd = sz.ChunkedCodec(codec, w // 8, D, chunk_len, device="cuda:0")
    with ran(only=[enc, *DENSE], never=ROUND6 if enc_fell else (), what=tag, **{enc: 1}):
        batch = cd.compress(to_device(cd, data))
    total = int(batch.offsets[-1].item())
    comp, offs, sizes = batch.data[:total].cpu().numpy(), batch.offsets.cpu().numpy(), batch.sizes.cpu().numpy()
    check_streams(oracle, codec, data, chunk_len, D, comp, offs, sizes, tag)
    if fixture is not None:
        m, want = fixture
        assert chunk_len == m["n"] and zlib.crc32(data[:chunk_len].tobytes()) == m["input_crc32"], (m, "not the fixture's input")
        assert np.array_equal(comp[offs[0]:offs[0] + sizes[0]], want), (tag, "differs from the compiled reference's bytes")
    decode_checked(cd, batch, data, chunk_len, nchunks, dec, dec_fell, tag + " own container")
    decode_checked(cd, oracle_batch(sz, oracle, codec, D, data, chunk_len), data, chunk_len, nchunks, dec, dec_fell, tag + " the oracle's container")


def roundtrip(sz, oracle, golden, codec, w, D, kind, nchunks, nblocks, r, enc, dec, tag):
    data, chunk_len, _ = batch_of(codec, w, D, kind, nchunks, nblocks, r)
    fixture = golden.get((codec, w, D, kind)) if (nchunks, nblocks, r) == (NCHUNKS, NB, 0) else None
    roundtrip_data(sz, oracle, codec, w, D, data, chunk_len, nchunks, enc, dec, f"{tag} [{codec} {kind} r={r}]", fixture)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_runs_through_every_edge_on_every_kernel(sz, oracle, golden, case):
    tag, codecs, opts, w, D, nchunks, nblocks, r, enc, dec = case
    with options(**opts):
        for codec in codecs:
            for kind in rd.KINDS:
                roundtrip(sz, oracle, golden, codec, w, D, kind, nchunks, nblocks, r, enc, dec, tag)


@pytest.mark.parametrize("w,D,nblocks,r", LAT_SINGLE)
def test_workgroup_per_chunk_kernels_on_chunks_that_are_no_whole_blocks(sz, oracle, w, D, nblocks, r):
    """every chunk of the 16-chunk batches as a call of its own: `<=` and `<` stop alike, and the verbatim tail is no whole pieces"""
    with options(**DEF):
        for codec in BOTH:
            for kind in rd.KINDS:
                data, chunk_len, _ = batch_of(codec, w, D, kind, NCHUNKS, nblocks, r)
                for c in range(NCHUNKS):
                    roundtrip_data(sz, oracle, codec, w, D, data[c * chunk_len:(c + 1) * chunk_len], chunk_len, 1, "enc_lat", "dec_lat",
                                   f"lat w={w} D={D} [{codec} {kind} r={r} chunk {c}]")


@pytest.mark.parametrize("codec", BOTH)
@pytest.mark.parametrize("case", CAP_CASES, ids=[c[0] for c in CAP_CASES])
def test_the_cap(sz, oracle, case, codec):
    """runs of 32 767, 32 767 and 4 466 blocks: the cap closes a run into the next slot and, in slot 1, opens a group with a run"""
    tag, opts, w, D, enc, dec = case
    data, chunk_len, zero = rd.cap_chunks(codec, w, D)
    cd = sz.ChunkedCodec(codec, w // 8, D, chunk_len, device="cuda:0")
    with options(**opts):
        with ran(only=[enc, *DENSE], what=tag, **{enc: 1}):
            batch = cd.compress(to_device(cd, data))
        total = int(batch.offsets[-1].item())
        comp, offs, sizes = batch.data[:total].cpu().numpy(), batch.offsets.cpu().numpy(), batch.sizes.cpu().numpy()
        check_streams(oracle, codec, data, chunk_len, D, comp, offs, sizes, tag)
        for c in range(3):
            got = rd.slots(comp[offs[c]:offs[c] + sizes[c]], w, D)
            assert got[2][:3] == [(0, 0, "run", rd.CAP), (0, 1, "run", rd.CAP), (1, 0, "run", 70000 - 2 * rd.CAP)], (tag, c, got[2])
            assert got == rd.model_slots(zero[c], chunk_len, D, 8, codec == "xff" and not rd.is_lowdim(w, D))
        decode_checked(cd, batch, data, chunk_len, 3, dec, False, tag + " own container")
        decode_checked(cd, oracle_batch(sz, oracle, codec, D, data, chunk_len), data, chunk_len, 3, dec, False, tag + " the oracle's container")


# ------------------------------------------------------------------ row operations over the same batches

                                                        # three -- runs of 1, 2, 4, 5 ... blocks start and end inside windows


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_query_windows_over_runs(sz, oracle, no_fast, chunks_per_group, codec, w, D, kind):
    cd, batch, data, chunk_len, _ = rowop_batch(sz, oracle, codec, w, D, kind)
    with options(**OLD):
        for W in WINDOWS:
            mn, mx, sums = wm.chunk_windows(data, chunk_len, D, W)
            for fam, cpg, family in legs(w, D, "window"):
                no_fast(fam)
                chunks_per_group(cpg)
                with ran(only=[family], **{family: 1}):
                    got = cd.query_windows(batch, W, per_chunk=True)
                msg = (codec, w, D, kind, W, family, cpg)
                assert np.array_equal(got["min"].cpu().numpy(), mn) and np.array_equal(got["max"].cpu().numpy(), mx), msg
                assert np.array_equal(got["sum"].cpu().numpy().view(np.uint64), sums), msg


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_filter_rows_over_runs(sz, oracle, no_fast, chunks_per_group, codec, w, D, kind):
    cd, batch, data, chunk_len, _ = rowop_batch(sz, oracle, codec, w, D, kind)
    sets, _ = bound_sets(data, chunk_len, w // 8, D)
    with options(**OLD):
        for name, mode, lo, hi, _ in sets:
            want = fm.filter_rows(data, chunk_len, D, lo, hi, mode)
            for fam, cpg, family in legs(w, D, "filter"):
                no_fast(fam)
                chunks_per_group(cpg)
                with ran(only=[family], **{family: 1}):
                    mask, counts = run_filter(cd, batch, lo, hi, mode)
                assert np.array_equal(counts, want[1]) and np.array_equal(mask, want[0]), (codec, w, D, kind, name, family, cpg)


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_select_rows_over_runs(sz, oracle, no_fast, chunks_per_group, codec, w, D, kind):
    cd, batch, data, chunk_len, zero = rowop_batch(sz, oracle, codec, w, D, kind)
    with options(**OLD):
        for name, mask in run_masks(zero, 11):
            cnt = sm.counts(mask, data.size, chunk_len, D)
            total = int(cnt.sum())
            assert 0 < total < data.size // D
            for fam, cpg, family in legs(w, D, "select"):
                no_fast(fam)
                chunks_per_group(cpg)
                with ran(only=[family], **{family: 1}):
                    check_select(data, batch, codec, w // 8, D, chunk_len, mask, sm.prefix_bases(cnt), total, total, (codec, w, D, kind, name, family, cpg))


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_aggregate_rows_over_runs(sz, oracle, no_fast, chunks_per_group, codec, w, D, kind):
    cd, batch, data, chunk_len, zero = rowop_batch(sz, oracle, codec, w, D, kind)
    with options(**OLD):
        for name, mask in run_masks(zero, 12):
            for W in WINDOWS:
                want = am.aggregate_rows(data, chunk_len, D, mask, W)
                for fam, cpg, family in legs(w, D, "aggregate"):
                    no_fast(fam)
                    chunks_per_group(cpg)
                    with ran(only=[family], **{family: 1}):
                        check_agg(data, batch, codec, w // 8, D, chunk_len, mask, W, (codec, w, D, kind, name, W, family, cpg), want)


def run_edge_starts(zero, rows):
    """batch rows at which a range begins: each run's first row, its last row, the row before the run and the row behind it"""
    R = 8 * zero.shape[1]
    starts = []
    for c, z in enumerate(zero):
        edges = np.flatnonzero(np.diff(np.concatenate([[0], z.astype(np.int8), [0]])))
        for a, b in zip(edges[::2], edges[1::2]):                       # blocks [a, b)
            starts += [c * R + 8 * a, c * R + 8 * b - 1, c * R + 8 * a - 1, c * R + 8 * b]
    total = zero.shape[0] * R
    return np.array(sorted({s for s in starts if 0 <= s <= total - rows}), np.int64)


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_gather_rows_over_runs(sz, oracle, no_fast, chunks_per_group, codec, w, D, kind):
    import torch
    cd, batch, data, chunk_len, zero = rowop_batch(sz, oracle, codec, w, D, kind)
    x = data.reshape(-1, D)
    with options(**OLD):
        for rows in (1, 11):
            starts = run_edge_starts(zero, rows)
            assert starts.size >= 4 * NCHUNKS
            want, ok = gm.expected(x, starts, rows)
            assert ok.all()
            for fam, cpg, family in legs(w, D, "gather"):          # (a gather's lane group serves one piece: the option must not reach it)
                no_fast(fam)
                chunks_per_group(cpg)
                rets = torch.full((starts.size,), -77, dtype=torch.int64, device="cuda:0")
                with ran(only=[family], **{family: 1}):
                    got = cd.gather_rows(batch, starts, rows, rets=rets)
                assert (rets.cpu().numpy() == rows).all(), (codec, w, D, kind, rows, family, cpg)
                bad = np.nonzero((got.cpu().numpy() != want).reshape(starts.size, -1).any(axis=1))[0]
                assert bad.size == 0, (codec, w, D, kind, rows, family, cpg, "ranges that begin at batch rows", starts[bad][:8].tolist())
