"""The tables of the run drive's and the FIRE drive's GPU tests (tests/rle_drive.py, tests/fire_drive.py): shapes, cases with the kernel family
each must run on, the masks, binnings, predicates and bands of the row operations, and the fixtures that hand a test a damaged batch.  The CPU
tier imports the same objects, so what it replays through the planner and checks for reach is what the GPU tier runs.  The fixtures here
ask for `sz`, `oracle`, `no_fast` and `chunks_per_group`: a module that takes one imports those from fixtures.py too."""
from functools import lru_cache

import numpy as np
import pytest

import fire_drive as fd
import linear_model as lm
import rle_drive as rd
import zone_model as zm
from dispatch import ROUND6
from rowdata import quartiles
from streams import DEF, GENERIC, OLD, fire_batch_of, fire_oracle_batch, options, truncated_batch


# ------------------------------------------------------------------ the run drive's

NCHUNKS, NB = 16, 256            # the fixture's batch: 16 rotations of 256 blocks (a 129-block run and every prefix)


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


# In a batch of more than one chunk, encode_lat.h and decode_lat.h take chunks of whole 16-byte pieces only (every chunk starts 16-byte
# aligned); a single chunk may end anywhere.  So r = 1 and r = 8 D - 1 reach them one chunk a call: w, ndims, blocks, r
LAT_SINGLE = [(8, 1, NB, 1), (8, 1, NB, 7), (16, 8, NB, 1), (16, 8, NB, 63), (8, 16, 192, 127)]


# id, options, w, ndims, encoder, decoder: 3 chunks of 70 000 all-zero blocks and two packed ones, on the family the planner assigns
CAP_CASES = [
    ("cap u8 D=1", OLD, 8, 1, "enc_uni", "dec_uni"),
    ("cap u8 D=5", OLD, 8, 5, "enc_generic", "dec_generic"),
]


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


# ------------------------------------------------------------------ the later row operations over both drives

def masks_for(zero, seed):
    """run_masks' three -- pseudo-random rows, exactly the rows inside runs, exactly the rows outside -- and no mask at all"""
    return run_masks(zero, seed) + [("none", None)]


def refs_for(D):
    """the moments' reference column: the first, a middle and the last one"""
    return (0, D // 2, D - 1)


def hist_binnings(w, D):
    """[(name, lo [D] or None, shift, nbins, chunks a histogram)]: the middle half of the range at full (8 bits) or 1 / 256 (16 bits)
    resolution -- the delta drive's columns walk out from 0 by amplitudes of their own, so a run's value lies inside the bins in some
    chunks and outside in others --, one histogram a batch; and bins of 4 (256) values over the whole range, a histogram every two
    chunks: at three chunks a lane group a histogram ends inside a group"""
    if w == 8:
        return [("clip", np.full(D, 64, np.int64), 0, 128, 0), ("shift", None, 2, 64, 2)]
    return [("clip", np.full(D, 0x4000, np.int64), 8, 128, 0), ("shift", None, 8, 256, 2)]


# group-by: the key column -- the first one behind column 0 that moves in at least 12 of the delta drive's 16 chunks (a column's
# amplitude is drawn per chunk, and 0 is one of the draws; tests/test_rowop_drive_cpu.py asserts it) -- and the bins: the middle half of
# the key's range, as the histogram's, so that whole runs are dropped in some chunks and counted in others
GBY_KEY = {(16, 8): 1, (8, 32): 1, (16, 12): 1}


def gby_binning(w):
    """(key_lo, shift, nbins)"""
    return (64, 0, 128) if w == 8 else (0x4000, 8, 128)


GBY_TABLES = (0, 2)                                    # chunks a table: one table; one every two chunks


def linear_sets(x, D, col):
    """[(name, w, u, bias, lo, hi)]: a sum over the row, a change of one column against the row in front (w + u = 0: a delta run's rows
    all have s = bias), and a lag term with w + u != 0 (a run's rows have s = sum (w + u) x: what the shortcut evaluates once).  The
    bounds are the quartiles of the model's sums, so that a predicate splits the rows; they are inputs, not tolerances"""
    e = np.eye(D, dtype=np.int64)
    ones = np.ones(D, np.int64)
    sets = []
    for name, w, u in (("ones", ones, None), ("change", e[col], -e[col]), ("w + u != 0", ones, 2 * e[col])):
        sets.append((name, w, u, 0) + quartiles(lm.sums(x, D, w, u)))
    return sets


LIN_COL = GBY_KEY                                      # the column whose change is asked for: one that moves


def zone_band(x, chunk_len, D, w):
    """-> (column, lo) of the band lo <= x[column] <= the type's maximum, every other column open: the first column, and for it the
    threshold, under which the zone map decides the most chunks while at least two are decided (a chunk whose column lies wholly above
    or wholly below lo) and at least two must be decoded -- or None where no such band exists.  Read off the model's map alone"""
    zmin, zmax, _ = zm.zone_map(x, chunk_len, D, w // 8)
    zmin, zmax = zmin.astype(np.int64), zmax.astype(np.int64)
    best = None
    for d in range(D):
        for lo in sorted(set((zmin[:, d] + 1).tolist()) | set(zmin[:, d].tolist()) | set((zmax[:, d] + 1).tolist())):
            if not 0 < lo < 1 << w:
                continue
            decided = int(((zmin[:, d] >= lo) | (zmax[:, d] < lo)).sum())
            if decided >= 2 and zmin.shape[0] - decided >= 2 and (best is None or decided > best[0]):
                best = (decided, d, int(lo))
        if best is not None:
            break
    return None if best is None else best[1:]


def band_bounds(band, w, D):
    """-> (lo [D], hi [D]) of filter_rows, (weights [D], lo, hi) of filter_linear: the same predicate twice"""
    d, t = band
    top = (1 << w) - 1
    lo, hi = np.zeros(D, np.int64), np.full(D, top, np.int64)
    lo[d] = t
    return (lo, hi), (np.eye(D, dtype=np.int64)[d], t, top)


BAD = 4                                                # at three chunks a group: the middle chunk of the second group
DAMAGE_SHAPES = [(codec, w, D) for codec in BOTH for (w, D) in ((16, 8), (8, 32))]       # (select rows needs rows of whole 16-byte pieces on decode_fast.h)
DAMAGE_IDS = [f"{c}-u{w}x{D}" for c, w, D in DAMAGE_SHAPES]


@pytest.fixture
def damaged(sz, oracle, no_fast, chunks_per_group):
    """-> f(codec, w, D): the "lengths" batch in the oracle's container with a wrong ndims in bytes 6 .. 7 of chunk 4's stream header, on
    decode_fast.h at three chunks a lane group.  The chunk is rejected before anything of it is parsed: its rets entry is negative, its
    own outputs are unspecified, and chunk 5 starts after a re-prime with its neighbours' state left in the registers"""
    import torch

    def make(codec, w, D):
        cd, batch, data, chunk_len, zero = rowop_batch(sz, oracle, codec, w, D, "lengths")
        off = int(batch.offsets[BAD].item())
        wrong = D ^ 5
        batch.data[off + 6:off + 8] = torch.tensor([wrong & 0xFF, wrong >> 8], dtype=torch.uint8, device="cuda")
        no_fast(0)
        chunks_per_group(3)
        return cd, batch, data, chunk_len, masks_for(zero, 31)[0][1]
    with options(**OLD):
        yield make


@pytest.fixture
def truncated(sz, oracle, no_fast, chunks_per_group):
    """-> f(codec, w, D): the "lengths" batch with chunk 4's stream cut short by 5 bytes and the streams packed densely again, as
    tests/test_gpu_extrema.py truncates them, on decode_fast.h at three chunks a lane group.  Unlike a header that is rejected, this
    chunk is decoded block by block and found damaged behind its last group: at a window of 64 rows its last window is then open, its
    rows and sums still in the registers -- what the chunk loop's reset has to clear before chunk 5"""
    def make(codec, w, D):
        cd, batch, data, chunk_len, zero = rowop_batch(sz, oracle, codec, w, D, "lengths")
        cut = truncated_batch(sz, batch, BAD)
        no_fast(0)
        chunks_per_group(3)
        return cd, cut, data, chunk_len, masks_for(zero, 32)[0][1]
    with options(**OLD):
        yield make


FIRE_SHAPES = {
    # (w, D): chunks, then (options, NO_FAST leg's chunks_per_group values, family) of every leg.  8 bits: every counter wraps, with run
    # spans at frozen extreme coefficients.  16 bits, one column: the low-dim coefficient passes 2^23; decode_uni.h is not taught these modes
    (8, 8): (7, [(OLD, 1, "dec_fast"), (OLD, 3, "dec_fast"), (GENERIC, 1, "dec_generic")]),
    (16, 1): (5, [(OLD, 1, "dec_generic")]),
}


FIRE_IDS = [f"u{w}x{D}" for w, D in FIRE_SHAPES]
FIRE_COL = 0                                           # the column whose change is asked for
PATCH_CHUNK, PATCH_TOP, PATCH_ZERO = 4, 140 * 64 + 13, 142 * 64 + 40        # (the middle chunk of the second group of three)


def fire_rows(w, D):
    return 8 * (fd.NB8 if w == 8 else fd.NB16)


def fire_windows(w, D):
    """64 rows, and one window a chunk"""
    return (64, fire_rows(w, D))


def three_of_8(nchunks, R):
    return np.full((nchunks, R // 8), 0b00100101, np.uint8)


@lru_cache(maxsize=None)
def fire_patched(w, D):
    """-> (samples, mask): a copy of the batch with one row of all ones in every column and one of zeros, in two windows of 64 rows of
    chunk 4, under the 3-of-8 mask with those two rows as their windows' only selected ones -- a selected all-ones value is a minimum
    with a row, a selected 0 a maximum with a row: the edges behind the extrema identities, whatever the drive gives"""
    nchunks = FIRE_SHAPES[(w, D)][0]
    data, chunk_len = fire_batch_of(w, D, nchunks)
    R = chunk_len // D
    x = data.copy().reshape(nchunks, R, D)
    x[PATCH_CHUNK, PATCH_TOP] = (1 << w) - 1
    x[PATCH_CHUNK, PATCH_ZERO] = 0
    mask = three_of_8(nchunks, R)
    for r in (PATCH_TOP, PATCH_ZERO):
        mask[PATCH_CHUNK, r // 64 * 8:r // 64 * 8 + 8] = 0
        mask[PATCH_CHUNK, r >> 3] = 1 << (r & 7)
    x = x.ravel()
    x.setflags(write=False)
    mask.setflags(write=False)
    return x, mask


def fire_batch(sz, oracle, w, D, data=None):
    nchunks = FIRE_SHAPES[(w, D)][0]
    x, chunk_len = fire_batch_of(w, D, nchunks)
    data = x if data is None else data
    cd = sz.ChunkedCodec("xff", w // 8, D, chunk_len, device="cuda:0")
    return cd, fire_oracle_batch(sz, oracle, D, data, chunk_len), data, chunk_len, nchunks


def fire_legs(sz, w, D, chunks_per_group):
    """every leg of the shape under its options: -> (family, chunks_per_group)"""
    for opts, cpg, family in FIRE_SHAPES[(w, D)][1]:
        with options(**opts):
            chunks_per_group(cpg)
            yield family, cpg


def fire_change_bounds(data, D):
    return quartiles(lm.sums(data, D, np.eye(D, dtype=np.int64)[FIRE_COL], -np.eye(D, dtype=np.int64)[FIRE_COL]))
