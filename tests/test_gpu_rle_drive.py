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
from functools import lru_cache

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
from test_gpu_aggregate import check_agg
from test_gpu_dispatch import check_streams
from test_gpu_filter import bound_sets, run_filter
from test_gpu_fire_extremes import DEF, DENSE, GENERIC, OLD, options, to_device
from test_gpu_select import check_select

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_rledrive_v1")
NCHUNKS, NB = 16, 256            # the fixture's batch: 16 rotations of 256 blocks (a 129-block run and every prefix)


@pytest.fixture(scope="module")
def sz():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sprintz_amd
    return sprintz_amd


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN + ".json") as f:
        manifest = json.load(f)["cases"]
    arrays = np.load(GOLDEN + ".npz")
    return {(m["codec"], m["w"], m["ndims"], m["kind"]): (m, arrays[m["name"]]) for m in manifest}


@lru_cache(maxsize=None)
def batch_of(codec, w, D, kind, nchunks, nblocks, r=0):
    """(flat samples, chunk_len, all-zero flags); read-only, shared by the cases of the module"""
    x, chunk_len, zero = rd.batch(codec, w, D, kind, nchunks, nblocks, r)
    x.setflags(write=False)
    return x, chunk_len, zero


def oracle_batch(sz, oracle, codec, D, data, chunk_len):
    """the ORACLE's streams as a container (16-byte aligned, as ChunkedCodec.compress builds it)"""
    import torch
    streams = oracle.compress_chunks(codec, data, chunk_len, D)
    offs = np.zeros(len(streams) + 1, np.int64)
    for c, s in enumerate(streams):
        offs[c + 1] = (offs[c] + s.size + 15) & ~15
    comp = np.zeros(int(offs[-1]) + sz._lib.READ_SLACK, np.uint8)
    for c, s in enumerate(streams):
        comp[offs[c]:offs[c] + s.size] = s
    return sz.CompressedBatch(torch.from_numpy(comp).cuda(), torch.from_numpy(offs).cuda(), torch.tensor([s.size for s in streams], dtype=torch.int32).cuda(),
                              len(streams), data.size, chunk_len, D)


def family_of(f):
    """a family literal, or ("falls through: why", the older family that must run instead)"""
    if isinstance(f, tuple):
        assert f[0].startswith("falls through: ") and f[1] not in ROUND6, f
        return f[1], True
    return f, False


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


BLK = dict(lat=0, blk_chunks=1, mask=7)                # encode_blk.h, decode_blk.h, encode_blk_uni
ROW = dict(lat=0, blk_chunks=1, mask=25)               # encode_blk.h, decode_row.h on every shape it fits
BOTH, DELTA = ("delta", "xff"), ("delta",)
PIECES = "falls through: encode_blk.h takes rows of whole 16-byte pieces"
TASKS = "falls through: encode_blk.h takes at most 256 (block, piece) tasks a chunk: 48 blocks x 16 pieces"
LOWDIM_DEC = "falls through: the low-dim layout has no block-parallel decoder (decode_uni.h)"

# id, codecs, options, w, ndims, chunks, blocks a chunk, elements behind the last whole block, encoder, decoder
CASES = [
    # ---- a workgroup per chunk (encode_lat.h: the scan formulation; decode_lat.h)
    ("lat u8 D=1", BOTH, DEF, 8, 1, NCHUNKS, NB, 0, "enc_lat", "dec_lat"),
    ("lat u16 D=8", BOTH, DEF, 16, 8, NCHUNKS, NB, 0, "enc_lat", "dec_lat"),
    ("lat u8 D=16: 192 blocks (24 KB: what the carve of 150 KB takes)", BOTH, DEF, 8, 16, NCHUNKS, 192, 0, "enc_lat", "dec_lat"),
    # ---- the low-dim layout, a lane per chunk (encode_uni.h, decode_uni.h)
    ("uni u8 D=1", BOTH, OLD, 8, 1, NCHUNKS, NB, 0, "enc_uni", "dec_uni"),
    ("uni u8 D=1 r=1", BOTH, OLD, 8, 1, NCHUNKS, NB, 1, "enc_uni", "dec_uni"),
    ("uni u8 D=1 r=7", BOTH, OLD, 8, 1, NCHUNKS, NB, 7, "enc_uni", "dec_uni"),
    ("uni u8 D=2", BOTH, OLD, 8, 2, NCHUNKS, NB, 0, "enc_uni", "dec_uni"),
    ("uni u8 D=3", BOTH, OLD, 8, 3, NCHUNKS, NB, 0, "enc_uni", "dec_uni"),
    ("uni u8 D=3 r=23", BOTH, OLD, 8, 3, NCHUNKS, NB, 23, "enc_uni", "dec_uni"),
    ("uni u8 D=4", BOTH, OLD, 8, 4, NCHUNKS, NB, 0, "enc_uni", "dec_uni"),
    ("uni u16 D=1", BOTH, OLD, 16, 1, NCHUNKS, NB, 0, "enc_uni", "dec_uni"),
    ("uni u16 D=2", BOTH, OLD, 16, 2, NCHUNKS, NB, 0, "enc_uni", "dec_uni"),
    ("uni u16 D=2 r=1", BOTH, OLD, 16, 2, NCHUNKS, NB, 1, "enc_uni", "dec_uni"),
    ("uni u16 D=2 r=15", BOTH, OLD, 16, 2, NCHUNKS, NB, 15, "enc_uni", "dec_uni"),
    # ---- the general layout, a lane per column or column pair (encode_wide.h, encode_fast.h; decode_fast.h)
    ("pair u16 D=8", BOTH, OLD, 16, 8, NCHUNKS, NB, 0, "enc_pair", "dec_fast"),
    ("fast u16 D=8 (ENC_PAIR 0)", BOTH, dict(OLD, pair=0), 16, 8, NCHUNKS, NB, 0, "enc_fast", "dec_fast"),
    ("pair u8 D=6", BOTH, OLD, 8, 6, NCHUNKS, NB, 0, "enc_pair", "dec_fast"),
    ("fast u8 D=6 (ENC_PAIR 0)", BOTH, dict(OLD, pair=0), 8, 6, NCHUNKS, NB, 0, "enc_fast", "dec_fast"),
    ("pair u8 D=32", BOTH, OLD, 8, 32, NCHUNKS, NB, 0, "enc_pair", "dec_fast"),
    ("fast u8 D=32 (ENC_PAIR 0)", BOTH, dict(OLD, pair=0), 8, 32, NCHUNKS, NB, 0, "enc_fast", "dec_fast"),
    ("split u8 D=80", BOTH, OLD, 8, 80, NCHUNKS, 51, 0, "enc_split", "dec_fast"),
    ("wide u8 D=96", BOTH, OLD, 8, 96, NCHUNKS, 48, 0, "enc_wide", "dec_fast"),
    ("wide u16 D=80", BOTH, OLD, 16, 80, NCHUNKS, 48, 0, "enc_wide", "dec_fast"),
    # ---- encode_kernel.h / decode_kernel.h: rows that are no whole 16-byte pieces, and everything under NO_FAST
    ("generic u8 D=5", BOTH, OLD, 8, 5, NCHUNKS, NB, 0, "enc_generic", "dec_generic"),
    ("generic u8 D=5 r=1", BOTH, OLD, 8, 5, NCHUNKS, NB, 1, "enc_generic", "dec_generic"),
    ("generic u8 D=5 r=39", BOTH, OLD, 8, 5, NCHUNKS, NB, 39, "enc_generic", "dec_generic"),
    ("generic u8 D=1 (NO_FAST)", BOTH, GENERIC, 8, 1, NCHUNKS, NB, 0, "enc_generic", "dec_generic"),
    ("generic u8 D=1 r=7 (NO_FAST)", BOTH, GENERIC, 8, 1, NCHUNKS, NB, 7, "enc_generic", "dec_generic"),
    ("generic u8 D=8 (NO_FAST)", BOTH, GENERIC, 8, 8, NCHUNKS, NB, 0, "enc_generic", "dec_generic"),
    ("generic u8 D=8 r=63 (NO_FAST)", BOTH, GENERIC, 8, 8, NCHUNKS, NB, 63, "enc_generic", "dec_generic"),
    # ---- more than 512 columns: a workgroup per chunk (any_ndims.hip); 2 chunks of 48 blocks
    ("any u8 D=600", BOTH, OLD, 8, 600, 2, 48, 0, "enc_any", "dec_any"),
    ("big u8 D=2048", BOTH, OLD, 8, 2048, 2, 48, 0, "enc_big", "dec_big"),
    # ---- the block-parallel delta kernels: rle_walk_scan over per-lane pieces (encode_blk.h), decode_blk.h, decode_row.h
    ("blk u8 D=16: 256 tasks", DELTA, BLK, 8, 16, NCHUNKS, NB, 0, "enc_blk", "dec_blk"),
    ("blk u8 D=80: 255 tasks", DELTA, BLK, 8, 80, NCHUNKS, 51, 0, "enc_blk", "dec_blk"),
    ("blk u16 D=8: 256 tasks", DELTA, BLK, 16, 8, NCHUNKS, NB, 0, "enc_blk", "dec_blk"),
    ("row u8 D=16", DELTA, ROW, 8, 16, NCHUNKS, NB, 0, "enc_blk", "dec_row"),
    ("row u8 D=80", DELTA, ROW, 8, 80, NCHUNKS, 51, 0, "enc_blk", "dec_row"),
    ("row u16 D=8", DELTA, ROW, 16, 8, NCHUNKS, NB, 0, "enc_blk", "dec_row"),
    ("row u8 D=12", DELTA, ROW, 8, 12, NCHUNKS, NB, 0, (PIECES, "enc_pair"), "dec_row"),
    ("row u8 D=256", DELTA, ROW, 8, 256, NCHUNKS, 48, 0, (TASKS, "enc_generic"), "dec_row"),
    ("blk_uni u8 D=1", DELTA, BLK, 8, 1, NCHUNKS, NB, 0, "enc_blk_uni", (LOWDIM_DEC, "dec_uni")),
    ("blk_uni u16 D=1", DELTA, BLK, 16, 1, NCHUNKS, NB, 0, "enc_blk_uni", (LOWDIM_DEC, "dec_uni")),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_runs_through_every_edge_on_every_kernel(sz, oracle, golden, case):
    tag, codecs, opts, w, D, nchunks, nblocks, r, enc, dec = case
    with options(**opts):
        for codec in codecs:
            for kind in rd.KINDS:
                roundtrip(sz, oracle, golden, codec, w, D, kind, nchunks, nblocks, r, enc, dec, tag)


# In a batch of more than one chunk, encode_lat.h and decode_lat.h take chunks of whole 16-byte pieces only (every chunk starts 16-byte
# aligned); a single chunk may end anywhere.  So r = 1 and r = 8 D - 1 reach them one chunk a call: w, ndims, blocks, r
LAT_SINGLE = [(8, 1, NB, 1), (8, 1, NB, 7), (16, 8, NB, 1), (16, 8, NB, 63), (8, 16, 192, 127)]


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


# id, options, w, ndims, encoder, decoder: 3 chunks of 70 000 all-zero blocks and two packed ones, on the family the planner assigns
CAP_CASES = [
    ("cap u8 D=1", OLD, 8, 1, "enc_uni", "dec_uni"),
    ("cap u8 D=5", OLD, 8, 5, "enc_generic", "dec_generic"),
]


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

# w, ndims -> the decoder family of: windows, filter, select, aggregate (csrc/plan.h: the reduce-only modes do not need rows of whole
# 16-byte pieces, select and gather do), and the gather family
# ... and of the later reduce-only modes -- histogram, moments, group-by, extrema, the linear filter -- with the tables of
# tests/test_gpu_rowop_drive.py (at most 128 x (D + 1) entries: 17 KB behind the groups' carves)
LATER = dict(histogram="dec_fast", moments="dec_fast", groupby="dec_fast", extrema="dec_fast", linear="dec_fast")
ROWOP_SHAPES = {
    (16, 8): dict(window="dec_fast", filter="dec_fast", select="dec_fast", aggregate="dec_fast", gather="gather_fast", **LATER),
    (8, 32): dict(window="dec_fast", filter="dec_fast", select="dec_fast", aggregate="dec_fast", gather="gather_fast", **LATER),
    (16, 12): dict(window="dec_fast", filter="dec_fast", select="dec_generic", aggregate="dec_fast", gather="gather_generic", **LATER),
}
ROWOP_KINDS = ("lengths", "start", "alternate", "tails")
ROWOP_CASES = [(codec, w, D, kind) for codec in BOTH for (w, D) in ROWOP_SHAPES for kind in ROWOP_KINDS]
ROWOP_IDS = [f"{c}-u{w}x{D}-{k}" for c, w, D, k in ROWOP_CASES]
WINDOWS = (8, 24)                                       # window_rows is a multiple of 8 at every entry point: one block a window, and
                                                        # three -- runs of 1, 2, 4, 5 ... blocks start and end inside windows


@pytest.fixture
def no_fast():
    from sprintz_amd import _lib

    def setter(v):
        _lib.check(_lib.set_option(_lib.OPT_NO_FAST, int(v)))
    yield setter
    _lib.set_option(_lib.OPT_NO_FAST, 1 if os.environ.get("SPRINTZ_MI355X_NO_FAST") is not None else 0)


@pytest.fixture
def chunks_per_group():
    """set_option(OPT_CHUNKS_PER_GROUP) for the duration of a test, restored afterwards"""
    from sprintz_amd import _lib

    def setter(k):
        _lib.check(_lib.set_option(_lib.OPT_CHUNKS_PER_GROUP, int(k)))
    yield setter
    _lib.set_option(_lib.OPT_CHUNKS_PER_GROUP, int(os.environ.get("SPRINTZ_MI355X_CHUNKS_PER_GROUP", 1)))


def rowop_batch(sz, oracle, codec, w, D, kind):
    """the ORACLE's container of the batch: expected values come from the models on the raw samples, never from a decode by the library"""
    data, chunk_len, zero = batch_of(codec, w, D, kind, NCHUNKS, NB)
    cd = sz.ChunkedCodec(codec, w // 8, D, chunk_len, device="cuda:0")
    return cd, oracle_batch(sz, oracle, codec, D, data, chunk_len), data, chunk_len, zero


def families(w, D, op):
    """(NO_FAST, family) pairs: the planner's family for the shape, then decode_kernel.h on the same batch"""
    first = ROWOP_SHAPES[(w, D)][op]
    generic = "gather_generic" if op == "gather" else "dec_generic"
    return [(0, first)] + ([(1, generic)] if first != generic else [])


CPGS = (1, 3)                                          # chunks a lane group of decode_fast.h: at 3 the 16 chunks fall to groups of 3, 3, 3, 3, 3 and 1


def legs(w, D, op):
    """(NO_FAST, chunks_per_group, family): the planner's family at one and at three chunks a lane group -- the chunk loop of
    decode_fast.h resets every mode's per-chunk state and reads ahead across the seam -- then decode_kernel.h, which ignores the
    option, once"""
    out = []
    for fam, family in families(w, D, op):
        out += [(fam, cpg, family) for cpg in (CPGS if family in ("dec_fast", "gather_fast") else CPGS[:1])]
    return out


def run_masks(zero, seed):
    """uint8 [nchunks, MB] in filter_rows' layout (8 rows a byte: a block a byte): pseudo-random rows, exactly the rows inside runs,
    exactly the rows outside"""
    rng = np.random.default_rng(seed)
    inside = np.where(zero, 0xFF, 0).astype(np.uint8)
    return [("random", rng.integers(0, 256, zero.shape).astype(np.uint8)), ("inside runs", inside), ("outside runs", ~inside)]


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
