"""CPU tier of segment rows (sprintz_mi355x_segment_count / _segment_rows, ChunkedCodec.segment_rows): the numpy model
(tests/segment_model.py) against a plain row loop, rowops.fold_segments on torch CPU tensors against the model of the batch taken as one
chunk, what the masks of tests/test_gpu_segments.py must reach -- asserted here without a device -- and the planner
(sprintz_amd/csrc/plan.h, built with g++: tests/plan_probe.cpp), which must give the mode what it gives aggregate rows."""
import os
import zlib

import numpy as np
import pytest

import dispatch_cases as dc
import filter_model as fm
import planner
import segment_model as sgm
from drive_tables import BOTH, NB, NCHUNKS, ROWOP_KINDS, ROWOP_SHAPES, batch_of, masks_for
from fixtures import random_mask
from planner import QUERY
from rowdata import MASKED_SHAPES as SHAPES, gen_data, parity_masks, rows_for, short_batch
from harness import DTYPES

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = (sgm.RUNS, sgm.SPLITS)
Q_AGGREGATE, Q_SEGMENT = QUERY["aggregate"], QUERY["segment"]
KEYS = ("counts", "chunk", "start", "rows", "min", "max", "sum")


def assert_same(a, b, msg):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (k,) + msg


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_model_against_a_row_loop(esz, mode):
    """random masks and lengths: full batches, a short last chunk of whole rows, one that ends mid-row, one chunk of a single row; R a
    multiple of 8 and not -- with random padding bits, and with all of them set"""
    rng = np.random.default_rng(100 * esz + mode)
    top = 1 << (8 * esz)
    for D, R in ((1, 16), (3, 13), (2, 24), (5, 9), (4, 8), (1, 1)):
        chunk_len = D * R
        MB = -(-R // 8)
        for nchunks in (1, 4):
            for n in {nchunks * chunk_len, (nchunks - 1) * chunk_len + D * max(1, R // 3), (nchunks - 1) * chunk_len + D * (R // 2) + D // 2, (nchunks - 1) * chunk_len + D} - {0}:
                x = rng.integers(0, top, n).astype(DTYPES[esz])
                for p in (0.0, 0.1, 0.5, 0.9, 1.0):
                    mask = random_mask(rng, -(-n // chunk_len), MB, p)               # (a length may leave the last chunk out)
                    want = sgm.segment_rows_brute(x, chunk_len, D, mask, mode)
                    assert_same(want, {k: sgm.segment_rows(x, chunk_len, D, mask, mode)[k] for k in KEYS}, (D, R, n, p))
                    if R % 8:
                        dirty = mask.copy()
                        dirty[:, -1] |= (0xFF << (R % 8)) & 0xFF
                        assert_same(want, {k: sgm.segment_rows(x, chunk_len, D, dirty, mode)[k] for k in KEYS}, (D, R, n, p, "padding set"))
                    lens = fm.chunk_counts(n, chunk_len)
                    assert np.array_equal(sgm.segment_count(mask, chunk_len, D, mode, lens), want["counts"]), (D, R, n, p)
                    assert np.array_equal(want["rows"].sum(), np.uint64(sgm.batch_bits(mask, n, chunk_len, D).sum() if mode == sgm.RUNS else n // D))


def test_the_definition_on_a_case_by_hand():
    x = np.arange(1, 13, dtype=np.uint8)                                          # one column, one chunk of 12 rows: values 1 .. 12
    mask = np.array([[0b01100111, 0b00001001]], np.uint8)                         # rows 0 1 2 . . 5 6 . 8 . . 11
    runs = sgm.segment_rows(x, 12, 1, mask, sgm.RUNS)
    assert runs["start"].tolist() == [0, 5, 8, 11] and runs["rows"].tolist() == [3, 2, 1, 1]
    assert runs["sum"].ravel().tolist() == [6, 13, 9, 12] and runs["min"].ravel().tolist() == [1, 6, 9, 12] and runs["max"].ravel().tolist() == [3, 7, 9, 12]
    splits = sgm.segment_rows(x, 12, 1, mask, sgm.SPLITS)                          # a set bit opens a segment: 0 | 1 | 2 3 4 | 5 | 6 7 | 8 9 10 | 11
    assert splits["start"].tolist() == [0, 1, 2, 5, 6, 8, 11] and splits["rows"].tolist() == [1, 1, 3, 1, 2, 3, 1]
    assert splits["sum"].ravel().tolist() == [1, 2, 12, 6, 15, 30, 12]
    clear = sgm.segment_rows(x, 12, 1, np.zeros((1, 2), np.uint8), sgm.SPLITS)    # no bit: row 0 still starts the one segment
    assert clear["start"].tolist() == [0] and clear["rows"].tolist() == [12] and sgm.segment_rows(x, 12, 1, np.zeros((1, 2), np.uint8), sgm.RUNS)["counts"].tolist() == [0]
    short = sgm.segment_rows(x[:7], 12, 1, mask, sgm.RUNS)                         # 7 rows exist: the run of rows 5, 6 ends with them
    assert short["start"].tolist() == [0, 5] and short["rows"].tolist() == [3, 2]
    assert sgm.segment_count(mask, 12, 1, sgm.RUNS).tolist() == [4] and sgm.segment_count(mask, 12, 1, sgm.RUNS, [7]).tolist() == [2]
    assert sgm.segment_count(mask, 12, 1, sgm.SPLITS, [-5]).tolist() == [0] and sgm.segment_count(mask, 12, 1, sgm.SPLITS, [100]).tolist() == [7]


def as_torch(m, dtype):
    """the model's per-chunk segments in the form ChunkedCodec.segment_rows hands to rowops.fold_segments"""
    import torch
    dt = torch.uint8 if dtype == np.uint8 else torch.uint16
    view = np.int8 if dtype == np.uint8 else np.int16
    res = {k: torch.from_numpy(m[k].view(view).copy()).view(dt) for k in ("min", "max")}
    res["sum"] = torch.from_numpy(m["sum"].astype(np.int64))
    res["start"] = torch.from_numpy(m["start"].astype(np.int64))
    res["rows"] = torch.from_numpy(m["rows"].astype(np.int64))
    return res, dt


def as_numpy(v, dtype):
    import torch
    if v.dtype in (torch.uint8, torch.uint16):
        return v.view(torch.int8 if v.dtype == torch.uint8 else torch.int16).numpy().view(dtype)
    return v.numpy()


def assert_fold(x, chunk_len, D, mask, mode, min_rows, msg):
    import torch
    from sprintz_amd import rowops
    res, dt = as_torch(sgm.segment_rows(x, chunk_len, D, mask, mode), x.dtype)
    got = rowops.fold_segments(res, torch.from_numpy(mask), chunk_len // D, "runs" if mode == sgm.RUNS else "splits", min_rows, dt)
    want = sgm.segment_rows_one_chunk(x, chunk_len, D, mask, mode, min_rows)
    assert set(got) == set(want), msg
    for k in want:
        gk = as_numpy(got[k], x.dtype)
        assert gk.shape == want[k].shape and np.array_equal(gk, want[k]), (k,) + msg
    return want


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_fold_segments(esz, mode):
    rng = np.random.default_rng(7 * esz + mode)
    top = 1 << (8 * esz)
    for D, R, nchunks in ((3, 24, 7), (1, 13, 5), (2, 8, 9)):
        chunk_len = D * R
        MB = -(-R // 8)
        n = chunk_len * (nchunks - 1) + D * max(1, R // 3)
        x = rng.integers(0, top, n).astype(DTYPES[esz])
        for p in (0.0, 0.05, 0.5, 0.95, 1.0):
            mask = random_mask(rng, nchunks, MB, p)
            for min_rows in (1, 2, R + 1):
                assert_fold(x, chunk_len, D, mask, mode, min_rows, (D, R, p, min_rows))


def test_fold_segments_edges():
    """a segment that spans three chunks; min_rows that only the stitched segment passes; a SPLITS mask whose chunk opens with a set bit"""
    D, R, nchunks = 2, 8, 5
    chunk_len = D * R
    x = np.arange(nchunks * chunk_len - 3 * D, dtype=np.uint16) * 7 % 1000
    bits = np.zeros((nchunks, R), bool)
    bits[0, 5:] = True                                                             # rows 5 .. 7 of chunk 0, all of chunks 1 and 2, rows 0 .. 1 of chunk 3
    bits[1] = bits[2] = True
    bits[3, :2] = True
    bits[3, 4] = True
    mask = sgm.pack_bits(bits)
    per_chunk = sgm.segment_rows(x, chunk_len, D, mask, sgm.RUNS)
    assert per_chunk["counts"].tolist() == [1, 1, 1, 2, 0]
    want = assert_fold(x, chunk_len, D, mask, sgm.RUNS, 1, ("three chunks",))
    assert want["start"].tolist() == [5, 28] and want["rows"].tolist() == [21, 1]
    assert int(want["sum"][0, 0]) == int(x.reshape(-1, D)[5:26, 0].astype(np.int64).sum())
    want = assert_fold(x, chunk_len, D, mask, sgm.RUNS, 9, ("min_rows",))          # no chunk-relative piece has 9 rows; the stitched one has 21
    assert want["start"].tolist() == [5] and int(per_chunk["rows"].max()) == 8
    assert assert_fold(x, chunk_len, D, mask, sgm.RUNS, 22, ("min_rows drops all",))["start"].size == 0
    # SPLITS: chunk 1 opens with a set bit (a new segment at the seam), chunk 2 with a clear one (the segment goes on over the seam)
    bits = np.zeros((nchunks, R), bool)
    bits[0, 3] = bits[1, 0] = bits[2, 6] = True
    mask = sgm.pack_bits(bits)
    want = assert_fold(x, chunk_len, D, mask, sgm.SPLITS, 1, ("splits",))
    assert want["start"].tolist() == [0, 3, 8, 22] and want["rows"].tolist() == [3, 5, 14, 15]
    none = assert_fold(x, chunk_len, D, np.zeros((nchunks, 1), np.uint8), sgm.SPLITS, 1, ("splits, no bit",))
    assert none["start"].tolist() == [0] and none["rows"].tolist() == [x.size // D]
    assert assert_fold(x, chunk_len, D, np.zeros((nchunks, 1), np.uint8), sgm.RUNS, 1, ("runs, no bit",))["start"].size == 0
    from sprintz_amd import rowops
    with pytest.raises(ValueError):
        rowops.fold_segments({}, None, 8, "windows", 1, None)


# ------------------------------------------------------------------ what the GPU tier's masks must reach

def gpu_masks(rng, x, chunk_len, esz, D):
    """the masks of tests/test_gpu_segments.py's parity and lane-mapping cases"""
    return parity_masks(rng, x, chunk_len, esz, D) + sgm.extra_masks(rng, x.size, chunk_len, D)


def test_the_gpu_masks_reach_the_edges():
    esz, D = 2, 8
    seen = set()
    for shape in SHAPES:
        R = rows_for(shape, D)
        chunk_len = R * D
        rng = np.random.default_rng(zlib.crc32(f"segments{shape}".encode()))
        x = gen_data("walk", rng, short_batch(5, chunk_len, D), esz, D)
        rows = sgm.chunk_rows(x.size, chunk_len, D)
        masks = dict(gpu_masks(rng, x, chunk_len, esz, D))
        assert len(masks) == 19 and rows[-1] < R                                   # the eleven of select's parity, and eight more
        for name, mask in masks.items():
            for mode in MODES:
                m = sgm.segment_rows(x, chunk_len, D, mask, mode)
                s, e = m["start"].astype(np.int64), m["start"].astype(np.int64) + m["rows"]
                # a segment that ends with row R - 1 of a chunk, followed by one that starts at the next chunk's row 0
                if np.any((e[:-1] % R == 0) & (s[1:] == e[:-1]) & (m["chunk"][1:] == m["chunk"][:-1] + 1)):
                    seen.add(("seam", mode))
                # four segments that start inside one mask byte
                if s.size and np.bincount(m["chunk"] * (-(-R // 8)) + (s % R) // 8).max() >= 4:
                    seen.add(("four a byte", mode))
                # a segment that lies wholly inside the verbatim tail: behind the chunk's last whole group of 16 rows
                tail0 = np.array([have // 16 * 16 if have >= 16 else 0 for have in rows])[m["chunk"]] + m["chunk"] * R
                if shape != "r16" and np.any((s > tail0) & (e < np.array(rows)[m["chunk"]] + m["chunk"] * R)):
                    seen.add(("inside the tail", mode, shape))
                if name == "padding alone":                                         # only bits of rows that do not exist: nothing under RUNS, one segment a chunk under SPLITS
                    assert m["counts"].tolist() == ([0] * 5 if mode == sgm.RUNS else [1] * 5) and (mask[:, -1] != 0).any()
        if R % 8:
            assert (masks["p=1/2, padding set"][:, -1] >> (R % 8)).all()
    for mode in MODES:
        assert ("seam", mode) in seen and ("four a byte", mode) in seen, seen
        assert ("inside the tail", mode, "tail") in seen and ("inside the tail", mode, "nogroups") in seen, seen
    assert dict(sgm.extra_masks(np.random.default_rng(0), 5 * 64, 64, 1))["0x55"][0, 0] == 0x55
    rb = sgm.ruler_bits(4000)
    s, e = sgm.edges(rb, sgm.RUNS)
    assert set((e - s).tolist()) == set(range(1, 18)) and len({int(a) % 8 for a in s}) == 8 and len({int(b) % 8 for b in e}) == 8


@pytest.mark.parametrize("codec,w,D", [(c, w, D) for c in BOTH for (w, D) in ROWOP_SHAPES])
def test_the_drive_masks_cut_runs_and_leave_runs_whole(codec, w, D):
    """over the drive's batches: under the masks of the GPU tier a run of zero blocks holds a start or an end in its mask bytes (the run is
    replayed block by block), and a run holds none (decode_fast.h's O(1) step), inside a segment and outside every segment"""
    seen = set()
    for kind in ROWOP_KINDS:
        data, chunk_len, zero = batch_of(codec, w, D, kind, NCHUNKS, NB)
        for name, mask in masks_for(zero, 41)[:3]:
            for mode in MODES:
                for c in range(NCHUNKS):
                    z = zero[c]
                    edges_ = np.flatnonzero(np.diff(np.concatenate([[0], z.astype(np.int8), [0]])))
                    for a, b in zip(edges_[::2].tolist(), edges_[1::2].tolist()):
                        bytes_ = mask[c, a:b]
                        open_ = (a > 0 and bool(mask[c, a - 1] >> 7)) if mode == sgm.RUNS else a > 0
                        if mode == sgm.RUNS:
                            plain = bool(np.all(bytes_ == (0xFF if open_ else 0)))
                        else:
                            plain = open_ and bool(np.all(bytes_ == 0))
                        seen.add((mode, "plain, inside" if plain and open_ else "plain, outside" if plain else "cut"))
    assert {(sgm.RUNS, "plain, inside"), (sgm.RUNS, "plain, outside"), (sgm.RUNS, "cut"), (sgm.SPLITS, "plain, inside"), (sgm.SPLITS, "cut")} <= seen, seen


# ------------------------------------------------------------------ the planner

@pytest.fixture(scope="module")
def plan():
    planner.available()
    return lambda queries: planner.ask_many(("decode", dict(q=Q_SEGMENT, **q) if "q" not in q else q) for q in queries)


def test_planner_gives_the_mode_what_it_gives_aggregate_rows(plan):
    """every shape of tests/dispatch_cases.py that aggregate_rows takes (the RLE codecs, whole rows, at most 512 columns), under the
    case's own options, both layouts, with and without OPT_NO_FAST, at one and three chunks a lane group: family, LDS, grid and mapping"""
    codes = {"delta": 0, "xff": 1}
    queries = []
    for case in dc.CASES:
        _, opts, codec, esz, D, chunk_len, nchunks = case[:7]
        if codec not in codes or chunk_len % D or D > 512:
            continue
        o = dict(dc.OPTION_DEFAULTS, **opts)
        for general in (0, 1):
            for no_fast in (0, 1):
                for cpg in (1, 3):
                    queries.append(dict(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=codes[codec], general=general, no_fast=no_fast,
                                        chunks_per_group=cpg, blk_chunks=o["blk_chunks"], lat_chunks=o["lat"]))
    assert len(queries) >= 200
    seg = plan([dict(q, q=Q_SEGMENT) for q in queries])
    agg = plan([dict(q, q=Q_AGGREGATE) for q in queries])
    assert seg == agg
    families = {got["family"] for got in seg}
    assert families == {"dec_fast", "dec_generic"}, families
    # the headline shape, and the low-dimension layouts: decode_uni.h is not taught the mode
    head = plan([dict(esz=2, D=8, chunk_len=5120, nchunks=131072, codec=1)])[0]
    assert head["family"] == "dec_fast" and head["dp"] == 8 and head["cpl"] == 1 and head["exact"] == 1
    low = [dict(esz=esz, D=D, chunk_len=cl, nchunks=4096, codec=1) for esz, D, cl in [(1, 1, 1024), (2, 1, 1024), (1, 2, 2048), (2, 2, 2048), (1, 3, 3000), (1, 4, 4096)]]
    assert all(got["family"] == "dec_generic" for got in plan(low))
    assert all(got["family"] == "dec_uni" for got in plan([dict(q, q=QUERY["window"]) for q in low]))
