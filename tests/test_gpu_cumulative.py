"""GPU tests (-m gpu) of cumulative rows (sprintz_mi355x_cumulative_rows, ChunkedCodec.cumulative_rows): per element, its column's running
min / max / sum from the batch's first row on, straight from a compressed batch.

The expected value is always the numpy model (tests/cumulative_model.py) on the ORIGINAL input, compared exactly -- every value is an
integer.  Every launch runs on 0xA5-filled outputs, scratch, carry and rets with guard bands around them (tests/cumulative_runner.py), and
asserts the kernel families of its launches (tests/dispatch.py) against the planner's answers for the shape (tests/plan_probe.cpp: q=17 for
the decode, q=3 for the totals pass)."""
import zlib

import numpy as np
import pytest

import cumulative_model as cm
import cumulative_runner as cr
import planner
from dispatch import ran
from drive_tables import ROWOP_CASES, ROWOP_IDS, fire_batch, rowop_batch
from drive_tables import FIRE_SHAPES as FIRE_TABLE
from fixtures import chunks_per_group, no_fast, sz  # noqa: F401  (fixtures)
from harness import DTYPES
from rowdata import FLOAT_FAST_SHAPES as FAST_SHAPES, GENERIC_SHAPES, RAGGED_SHAPES, gen_data, lowdim, make_batch
from streams import OLD, options, truncated_batch

pytestmark = pytest.mark.gpu

TILE = cm.SCAN_TILE


@pytest.fixture(scope="module")
def plan():
    """the planner on a host compiler: -> f(q=..., **fields) -> the answer"""
    planner.available(required=True)
    return lambda **fields: planner.ask("decode", **fields)


def rotate(key, k):
    return zlib.crc32(key.encode()) % k


def launch(plan, batch, x, codec, esz, D, chunk_len, ops, sb, msg, carry=None, general=False, no_fast=0, cpg=1, shift=0, expect=None, bad=(), **kw):
    """one call: the planner's families ran and nothing else, the results are the model's.  -> (the decode's family, the result)"""
    family, counts = cr.launches(plan, codec, esz, D, chunk_len, batch.nchunks, ops, sb, general, no_fast, cpg, (shift * esz) % 16)
    if expect is not None:
        assert family == expect, (family, expect) + msg
    with ran(only=list(counts), **counts):
        res = cr.run(batch, codec, esz, D, chunk_len, ops, sb, carry, general, shift, **kw)
    cr.check(res, x, chunk_len, batch.nchunks, D, ops, sb, msg + (family,), carry, shift, bad)
    return family, res


# ------------------------------------------------------------------ parity

def named_rows(esz, D):
    """24 .. 40 rows a chunk: 40 for the shapes named for decode_fast.h (its read-ahead ring takes u16 x 8, x 16 and x 64 from 37 / 38 rows on),
    24 .. 39 -- a group and a verbatim tail of 8 .. 23 rows -- for the others"""
    return 40 if (esz, D) in FAST_SHAPES else 24 + D % 16


@pytest.mark.parametrize("codec,esz,D", [(codec, esz, D) for codec in ("delta", "xff") for esz, D in FAST_SHAPES + GENERIC_SHAPES])
def test_cumulative_rows_parity_named_shapes(sz, oracle, no_fast, chunks_per_group, plan, codec, esz, D):
    """the sixteen shapes named for the planner, both codecs, both families (NO_FAST), 1 and 3 chunks a lane group, with and without the general
    layout, sum_bytes 4 and 8, with and without seeds; every subset of the ops on u16 x 8; 7 .. 9 chunks, the last one short and ending
    mid-row and mid-block"""
    key = f"cum{codec}{esz}{D}"
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    chunk_len = D * named_rows(esz, D)
    nchunks = 7 + D % 3
    n = (nchunks - 1) * chunk_len + 13 * D + D // 2
    x = gen_data(("walk", "uniform", "sparse")[rotate(key, 3)], rng, n, esz, D)
    batches = {False: make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)[1]}
    batches[True] = make_batch(sz, oracle, codec, esz, D, chunk_len, x, True)[1] if lowdim(esz, D) else batches[False]
    seen = set()
    for general in (False, True):
        for fam in (0, 1):
            no_fast(fam)
            for cpg in ((1, 3) if fam == 0 else (1,)):
                chunks_per_group(cpg)
                for sb in (4, 8):
                    for ops in (cm.SUBSETS if (esz, D, fam, cpg, general) == (2, 8, 0, 1, False) else (7,)):
                        carry = cr.random_carry(rng, D, esz) if (sb + cpg + fam) % 2 else None
                        family, _ = launch(plan, batches[general], x, codec, esz, D, chunk_len, ops, sb, (codec, esz, D, general, fam, cpg, sb, ops), carry, general, fam, cpg)
                        assert family == ("dec_fast" if cm.fast_takes(esz, D, chunk_len, general, fam, 0, cm.out_esz(esz, ops, sb)) else "dec_generic")
                        seen.add(family)
    assert ("dec_fast" in seen) == ((esz, D) in ((2, 8), (2, 16), (2, 64))) and "dec_generic" in seen
    chunks_per_group(1)


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz,D", [(1, 16), (2, 24), (1, 64), (1, 32)])
def test_cumulative_rows_parity_fast_shapes_at_48_rows(sz, oracle, chunks_per_group, plan, codec, esz, D):
    """the shapes of decode_fast.h whose ring needs more than 40 rows -- every 8-bit one among them: the sum's four and eight planes"""
    rng = np.random.default_rng(D + esz)
    chunk_len, nchunks = D * 48, 7
    n = (nchunks - 1) * chunk_len + 21 * D + D // 2
    x = gen_data("walk" if codec == "xff" else "uniform", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    for cpg in (1, 3):
        chunks_per_group(cpg)
        for sb, ops in ((8, 7), (4, 7), (8, 4), (4, 5)):
            launch(plan, batch, x, codec, esz, D, chunk_len, ops, sb, (codec, esz, D, cpg, sb, ops), cr.random_carry(rng, D, esz), cpg=cpg, expect="dec_fast")
    chunks_per_group(1)


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz,D,chunk_len,n", RAGGED_SHAPES)
def test_cumulative_rows_parity_ragged_shapes(sz, oracle, no_fast, plan, codec, esz, D, chunk_len, n):
    """whole rows, short last chunks (one ending mid-row), R % 8 != 0 and R < 8"""
    rng = np.random.default_rng(n)
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    for fam in (0, 1):
        no_fast(fam)
        for sb in (4, 8):
            launch(plan, batch, x, codec, esz, D, chunk_len, 7, sb, (codec, esz, D, chunk_len, fam, sb), cr.random_carry(rng, D, esz) if sb == 4 else None, no_fast=fam)


# ------------------------------------------------------------------ the scan across its tiles

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 3)])
@pytest.mark.parametrize("nchunks", [2 * TILE + 1, TILE - 1, TILE], ids=["2T+1", "T-1", "T"])
def test_cumulative_rows_scan_across_its_tiles(sz, oracle, plan, codec, esz, D, nchunks):
    """the smallest chunk (16 rows) and as many chunks as two tiles of the scan and one more, one tile less one, one tile: every chunk's
    level differs from its neighbours', columns rise and fall in turn, so that each chunk's entering state is its own"""
    rng = np.random.default_rng(nchunks + D)
    R = 16
    chunk_len = D * R
    n = nchunks * chunk_len - 5 * D
    top = 1 << (8 * esz)
    g = np.arange(nchunks * R, dtype=np.int64)[:, None]
    level = (g // R) * (3 if esz == 2 else 1) // (1 if esz == 2 else 40)
    noise = rng.integers(0, 7, (nchunks * R, D))
    m = np.where(np.arange(D)[None, :] % 2 == 0, level + noise, top - 1 - level - noise)
    assert m.min() >= 0 and m.max() < top
    x = m.astype(DTYPES[esz]).reshape(-1)[:n]
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    assert batch.nchunks == nchunks
    carry = cr.random_carry(rng, D, esz)
    launch(plan, batch, x, codec, esz, D, chunk_len, 7, 8, (codec, esz, D, nchunks), carry)
    want, _ = cm.cumulative(x, D, carry)
    first = np.arange(nchunks) * chunk_len + 1 % D                                 # (the data's own rule: the entering states differ from chunk to chunk)
    assert np.unique(want["sum"][first]).size == nchunks


# ------------------------------------------------------------------ the carry

@pytest.mark.parametrize("codec,esz,D,R", [("xff", 2, 8, 40), ("delta", 1, 16, 48), ("delta", 2, 5, 27), ("xff", 1, 1, 33)])
def test_cumulative_rows_carry_chains_batches(sz, oracle, plan, codec, esz, D, R):
    """one batch in one call against the same data as two batches, and as three, chained through carry_out -> carry_in; carry_out alone
    against the model's final state; a cut at a chunk seam and cuts inside a chunk"""
    rng = np.random.default_rng(R * D)
    chunk_len, nchunks = D * R, 7
    n = nchunks * chunk_len - 3 * D
    x = gen_data("walk", rng, n, esz, D)
    cd, whole = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    for seed in (None, cr.random_carry(rng, D, esz)):
        for sb in (8, 4):
            _, one = launch(plan, whole, x, codec, esz, D, chunk_len, 7, sb, (codec, esz, D, sb, "one call"), seed)
            body = {k: v[cr.PAD:cr.PAD + n] for k, v in one.outs.items()}
            for cuts in ([3 * R], [2 * R + 5], [R - 1, 4 * R + 9]):
                carry, parts, lo = seed, [], 0
                for hi in cuts + [n // D]:
                    piece = x[lo * D:hi * D]
                    _, b = make_batch(sz, oracle, codec, esz, D, chunk_len, piece, False)
                    _, res = launch(plan, b, piece, codec, esz, D, chunk_len, 7, sb, (codec, esz, D, sb, cuts, lo), carry)
                    carry = res.carry
                    parts.append({k: v[cr.PAD:cr.PAD + piece.size] for k, v in res.outs.items()})
                    lo = hi
                for k in body:
                    assert np.array_equal(np.concatenate([p[k] for p in parts]), body[k]), (k, cuts, sb)
                assert np.array_equal(carry, one.carry), (cuts, sb)
    # without carry_out nothing is written there (cumulative_runner.run checks the buffer), and the outputs are the same
    _, res = launch(plan, whole, x, codec, esz, D, chunk_len, 7, 8, (codec, esz, D, "no carry_out"), None, with_carry_out=False)
    assert res.carry is None


@pytest.mark.parametrize("codec,esz,D,chunks", [("xff", 2, 8, 4), ("delta", 2, 8, 1), ("delta", 1, 16, 4), ("xff", 2, 3, 2), ("delta", 1, 1, 1)])
def test_cumulative_rows_sum_crosses_its_wraps(sz, oracle, plan, codec, esz, D, chunks):
    """seeds of 2^32 - 5, 2^40 and 2^63 - 1 (and 2^64 - 3): within 64 rows of all-ones data the int64 sum and the int32 low half both cross
    their wraps, in one chunk and over the chunk seams"""
    R = 64 // chunks
    chunk_len = D * R
    x = np.full(64 * D, (1 << (8 * esz)) - 1, DTYPES[esz])
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    assert batch.nchunks == chunks
    seed = cm.identity(D, esz)
    seed[2] = np.array([(1 << 32) - 5, 1 << 40, (1 << 63) - 1, (1 << 64) - 3], dtype=np.uint64)[np.arange(D) % 4]
    for sb in (8, 4):
        _, res = launch(plan, batch, x, codec, esz, D, chunk_len, 4, sb, (codec, esz, D, chunks, sb), seed)
        got = res.outs["sum"][cr.PAD:cr.PAD + x.size]
        if sb == 8 and D >= 3:
            assert got[2] < 0 and np.all(got[2::D][:1] == np.int64(-(1 << 63)) + ((1 << (8 * esz)) - 2))      # 2^63 - 1 + top wraps to the bottom
        if sb == 4:
            assert got[0] == ((1 << (8 * esz)) - 1) - 5                                                      # 2^32 - 5 + top, low half


# ------------------------------------------------------------------ min / max edges

def ramp(esz, D, G, falling):
    """a strictly falling (rising) ramp down every column, another phase a column: the minimum (maximum) changes every row, the other never"""
    r = np.arange(G, dtype=np.int64)[:, None] + 3 * np.arange(D, dtype=np.int64)[None, :]
    top = (1 << (8 * esz)) - 1
    assert r.max() <= top
    return (top - r if falling else r).astype(DTYPES[esz]).reshape(-1)


@pytest.mark.parametrize("codec,esz,D,R", [("delta", 2, 8, 40), ("xff", 2, 8, 40), ("xff", 1, 16, 48), ("delta", 1, 3, 24), ("xff", 2, 5, 31)])
@pytest.mark.parametrize("kind", ["falling", "rising", "ones", "zeros", "spike"])
def test_cumulative_rows_min_max_edges(sz, oracle, plan, codec, esz, D, R, kind):
    top = (1 << (8 * esz)) - 1
    chunk_len, nchunks = D * R, 7
    G = nchunks * R - 6
    if esz == 1:
        nchunks = min(nchunks, (top - 3 * D) // R)
        G = nchunks * R - 6
    if kind in ("falling", "rising"):
        x = ramp(esz, D, G, kind == "falling")
    elif kind == "ones":
        x = np.full(G * D, top, DTYPES[esz])
    else:
        x = np.zeros(G * D, DTYPES[esz])
        if kind == "spike":
            x[(2 * R + 11) * D + D // 2] = top                                  # one sample, in one column, in chunk 2
            x[:D] = 7
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    _, res = launch(plan, batch, x, codec, esz, D, chunk_len, 7, 8, (codec, esz, D, kind))
    body = {k: v[cr.PAD:cr.PAD + x.size] for k, v in res.outs.items()}
    d = np.arange(x.size) % D
    if kind == "falling":
        assert np.array_equal(body["min"], x) and np.array_equal(body["max"], x[d])
    if kind == "rising":
        assert np.array_equal(body["max"], x) and np.array_equal(body["min"], x[d])
    # seeds tighter than the data: the output never leaves the seed
    tight = cm.identity(D, esz)
    tight[0], tight[1] = 0, top
    _, res = launch(plan, batch, x, codec, esz, D, chunk_len, 3, 8, (codec, esz, D, kind, "tight"), tight)
    assert not res.outs["min"][cr.PAD:cr.PAD + x.size].any() and np.all(res.outs["max"][cr.PAD:cr.PAD + x.size] == top)
    assert np.array_equal(res.carry, tight)


# ------------------------------------------------------------------ run paths

@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_cumulative_rows_over_runs(sz, oracle, chunks_per_group, plan, codec, w, D, kind):
    """tests/rle_drive.py's batches: runs of 1 .. 16 blocks and maximal ones, beginning at chunk starts and ending at the chunk's last block; on
    the planner's family for the shape (decode_fast.h at 1 and 3 chunks a lane group for u16 x 8 and u8 x 32)"""
    cd, batch, data, chunk_len, _ = rowop_batch(sz, oracle, codec, w, D, kind)
    with options(**OLD):
        for cpg in (1, 3):
            chunks_per_group(cpg)
            for sb, ops in ((8, 7), (4, 6)):
                launch(plan, batch, data, codec, w // 8, D, chunk_len, ops, sb, (codec, w, D, kind, cpg, sb), cpg=cpg, expect="dec_fast" if D != 12 else "dec_generic")
    chunks_per_group(1)


@pytest.mark.parametrize("w,D", list(FIRE_TABLE), ids=[f"u{w}x{D}" for w, D in FIRE_TABLE])
def test_cumulative_rows_on_the_fire_drive(sz, oracle, no_fast, plan, w, D):
    """tests/fire_drive.py's batches: FIRE counters through their int16 wrap, runs replayed at frozen extreme coefficients"""
    cd, batch, data, chunk_len, nchunks = fire_batch(sz, oracle, w, D)
    with options(**OLD):
        for fam in (0, 1):
            no_fast(fam)
            for sb, ops in ((8, 7), (4, 5)):
                launch(plan, batch, data, "xff", w // 8, D, chunk_len, ops, sb, ("fire", w, D, fam, sb), no_fast=fam)


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz,D", [(2, 8), (1, 3), (2, 1), (1, 32)])
def test_cumulative_rows_settled_runs(sz, oracle, plan, codec, esz, D):
    """constant columns long enough to enter a settled run mid-chunk and leave it at the chunk's end; a chunk that is one run; a step between
    two runs"""
    rng = np.random.default_rng(esz * 100 + D)
    R, nchunks = 16 * 9, 4
    chunk_len = D * R
    rows = np.zeros((nchunks, R, D), np.int64)
    rows[0, :] = 7 + np.arange(D)                                                  # one run, the whole chunk
    for c, moving in ((1, 37), (2, 64), (3, 5)):
        rows[c, :moving] = rng.integers(0, 200, (moving, D))
        rows[c, moving:] = 50 + c + np.arange(D)                                   # a run to the chunk's end ...
        rows[c, moving + 40:] += 3                                                 # ... with a step 40 rows into it
    x = rows.reshape(-1).astype(DTYPES[esz])
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    for sb, ops in ((8, 7), (4, 7), (8, 2)):
        launch(plan, batch, x, codec, esz, D, chunk_len, ops, sb, (codec, esz, D, sb, ops), cr.random_carry(rng, D, esz))


# ------------------------------------------------------------------ the ragged end, the edges of the buffers

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 16), ("delta", 2, 5), ("xff", 1, 7)])
def test_cumulative_rows_ragged_end_and_single_chunks(sz, oracle, plan, codec, esz, D):
    """a one-chunk batch without scratch (d_tmp NULL), full and ending mid-row and mid-block; a one-element batch; with and without seeds and
    carry_out: the decode launch alone reads the seeds and writes the carry"""
    rng = np.random.default_rng(5 * D)
    chunk_len = D * 48
    for n in (chunk_len, chunk_len - 2 * D - D // 2, 19 * D + D // 2, 1):
        x = gen_data("walk", rng, n, esz, D)
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        assert batch.nchunks == 1
        for sb in (8, 4):
            for seed in (None, cr.random_carry(rng, D, esz)):
                family, res = launch(plan, batch, x, codec, esz, D, chunk_len, 7, sb, (codec, esz, D, n, sb), seed, with_tmp=False)
                launch(plan, batch, x, codec, esz, D, chunk_len, 5, sb, (codec, esz, D, n, sb, "no carry_out"), seed, with_tmp=False, with_carry_out=False)
        assert family == ("dec_fast" if (esz, D) in ((2, 8), (1, 16)) else "dec_generic")
    # the columns a one-element batch lacks keep their seeds in carry_out
    assert np.array_equal(res.carry[:, 1:], cm.seeds(seed, D, esz)[:, 1:])


@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 16), ("delta", 2, 5), ("xff", 1, 7)])
def test_cumulative_rows_edges_of_the_buffers(sz, oracle, plan, codec, esz, D):
    """outputs off the 16-byte grid by one element and by 16 (the planner then sends the call to the generic kernel where it must), a last
    chunk that ends mid-row; every subset of the ops with the other outputs NULL: nothing is written outside the outputs, nor past the last
    chunk's count, and d_rets keeps the sentinel behind it"""
    rng = np.random.default_rng(7 * D)
    chunk_len, nchunks = D * 48, 7
    n = (nchunks - 1) * chunk_len + D * 37 + max(1, D // 2)
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    seen = set()
    for shift in (0, 1, 16):
        for sb, ops in ((8, 7), (4, 1), (4, 4), (8, 6)):
            family, _ = launch(plan, batch, x, codec, esz, D, chunk_len, ops, sb, (codec, esz, D, shift, sb, ops), None, shift=shift)
            seen.add((shift, family))
    if (esz, D) in ((2, 8), (1, 16)):
        assert (0, "dec_fast") in seen and (1, "dec_generic") in seen and (1, "dec_fast") not in seen


# ------------------------------------------------------------------ damage

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 32), ("delta", 2, 12)])
@pytest.mark.parametrize("cut", [0, 3, 6], ids=["first", "middle", "last"])
def test_cumulative_rows_damaged_chunk(sz, oracle, chunks_per_group, plan, codec, esz, D, cut):
    """one truncated chunk: d_rets is decompress_batch's; every chunk in front is exact, every chunk behind equals the model with the damaged
    chunk removed, carry_out likewise; nothing is written outside the outputs (the damaged chunk's own slot is not looked at)"""
    import torch
    rng = np.random.default_rng(3 * D + cut)
    chunk_len, nchunks = D * 48, 7
    n = nchunks * chunk_len - 5 * D
    x = gen_data("walk", rng, n, esz, D)
    cd, good = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    batch = truncated_batch(sz, good, cut)
    with options(**OLD):
        for cpg in (1, 3):
            chunks_per_group(cpg)
            plain_rets = torch.full((nchunks,), -77, dtype=torch.int64, device="cuda")
            cd.decompress(batch, rets=plain_rets)
            plain_rets = plain_rets.cpu().numpy()
            assert plain_rets[cut] < 0 and np.all(np.delete(plain_rets, cut) > 0)
            for sb, ops in ((8, 7), (4, 5)):
                seed = cr.random_carry(rng, D, esz)
                _, res = launch(plan, batch, x, codec, esz, D, chunk_len, ops, sb, (codec, esz, D, cut, cpg, sb), seed, cpg=cpg, bad=(cut,))
                assert np.array_equal(res.rets[:nchunks], plain_rets), (res.rets.tolist(), plain_rets.tolist())
                # the model with the chunk absent is the model of the batch without it
                rest = np.concatenate([x[:cut * chunk_len], x[(cut + 1) * chunk_len:]])
                assert np.array_equal(res.carry, cm.cumulative(rest, D, seed, ops)[1])
        with pytest.raises(sz.SprintzError, match=f"cumulative_rows: chunk {cut} "):
            cd.cumulative_rows(batch)
        got = cd.cumulative_rows(batch, check=False)
        assert got["sum"].shape == (n // D, D)
        cd.cumulative_rows(good)                                                   # undamaged: no error
    chunks_per_group(1)


def test_cumulative_rows_damaged_single_chunk(sz, oracle, plan):
    """a call of one chunk, damaged: carry_out is the seeds"""
    rng = np.random.default_rng(9)
    for codec, esz, D in (("xff", 2, 8), ("delta", 1, 5)):
        chunk_len = D * 48
        x = gen_data("walk", rng, chunk_len, esz, D)
        cd, good = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        batch = truncated_batch(sz, good, 0)
        seed = cr.random_carry(rng, D, esz)
        _, res = launch(plan, batch, x, codec, esz, D, chunk_len, 7, 8, (codec, esz, D), seed, bad=(0,), with_tmp=False)
        assert np.array_equal(res.carry, seed)


# ------------------------------------------------------------------ side stream, repeat, an empty batch

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 7)])
def test_cumulative_rows_side_stream_and_repeat(sz, oracle, plan, codec, esz, D):
    """the call on a non-default stream, twice in a row into the same buffers with dirty scratch: identical results"""
    import torch
    rng = np.random.default_rng(D)
    chunk_len, nchunks = D * 40, 9
    n = nchunks * chunk_len - 7 * D - D // 2
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    seed = cr.random_carry(rng, D, esz)
    side = torch.cuda.Stream()
    family, counts = cr.launches(plan, codec, esz, D, chunk_len, nchunks, 7, 8)
    with ran(only=list(counts), **{k: 2 * v for k, v in counts.items()}):
        first = cr.run(batch, codec, esz, D, chunk_len, 7, 8, seed, stream=side)
        snap = {k: v.copy() for k, v in first.outs.items()}
        again = cr.run(batch, codec, esz, D, chunk_len, 7, 8, seed, stream=side, bufs=first.bufs)
    cr.check(again, x, chunk_len, nchunks, D, 7, 8, (codec, esz, D, "again"), seed)
    assert all(np.array_equal(snap[k], again.outs[k]) for k in snap) and np.array_equal(first.carry, again.carry)


def test_cumulative_rows_empty_batch(sz):
    """nchunks == 0: nothing is decoded, carry_out receives the seeds -- the identities without carry_in"""
    import ctypes as C
    import torch
    from sprintz_amd import _lib
    for esz, D in ((2, 8), (1, 3)):
        dummy = torch.zeros(64, dtype=torch.int64, device="cuda")
        cout = torch.full((3 * D + 2,), 0x5A, dtype=torch.int64, device="cuda")
        seed = cr.random_carry(np.random.default_rng(D), D, esz)
        cin = torch.from_numpy(seed.view(np.int64)).cuda()
        for given, want in ((cin, seed), (None, cm.identity(D, esz))):
            with ran(only=[]):
                _lib.check(_lib.cumulative_rows(1, esz, dummy.data_ptr(), dummy.data_ptr(), 0, D * 16, D, 7, 8, 0, dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(),
                                                None if given is None else given.data_ptr(), cout.data_ptr() + 8, None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            got = cout.cpu().numpy()
            assert got[0] == 0x5A and got[-1] == 0x5A and np.array_equal(got[1:-1].view(np.uint64).reshape(3, D), want)


# ------------------------------------------------------------------ Python

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 5)])
def test_cumulative_rows_python(sz, oracle, plan, codec, esz, D):
    import torch
    rng = np.random.default_rng(11 * D)
    chunk_len = D * 40
    n = 6 * chunk_len + 20 * D + D // 2                                            # a partial last row
    x = gen_data("uniform", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    G = -(-n // D)
    view = torch.int8 if esz == 1 else torch.int16

    def flat(t):
        return t.cpu().numpy().reshape(-1)
    want, left = cm.cumulative(x, D)
    _, counts = cr.launches(plan, codec, esz, D, chunk_len, batch.nchunks, 7, 8)
    with ran(only=list(counts), **counts):                                         # one library call: the totals, the scan and the decode
        got, carry = cd.cumulative_rows(batch, ops=("min", "max", "sum", "mean"), return_carry=True)
    assert list(got) == ["min", "max", "sum", "mean"] and all(v.shape == (G, D) and v.device.type == "cuda" for v in got.values())
    assert got["min"].dtype == got["max"].dtype == cd.dtype and got["sum"].dtype == torch.int64 and got["mean"].dtype == torch.float64
    for k in ("min", "max"):
        assert np.array_equal(flat(got[k].view(view)).view(DTYPES[esz])[:n], want[k]) and not flat(got[k].view(view))[n:].any()
    assert np.array_equal(flat(got["sum"])[:n], cm.int64(want["sum"])) and not flat(got["sum"])[n:].any()
    assert np.array_equal(flat(got["mean"])[:n], cm.mean(want["sum"], D)) and not flat(got["mean"])[n:].any()
    assert carry.rows == G and np.array_equal(carry.table.cpu().numpy().view(np.uint64), left)
    # defaults; one op by name; the mean alone comes from the sum launch; the int32 sum is the low half; int32 and the mean are refused together
    assert list(cd.cumulative_rows(batch)) == ["min", "max", "sum"]
    only = cd.cumulative_rows(batch, ops="mean", general_layout=True)
    assert list(only) == ["mean"] and torch.equal(only["mean"], got["mean"])
    assert torch.equal(cd.cumulative_rows(batch, ops=("max",))["max"].view(view), got["max"].view(view))
    low = cd.cumulative_rows(batch, ops=("sum",), sum_dtype=torch.int32)["sum"]
    assert low.dtype == torch.int32 and np.array_equal(flat(low)[:n], cm.low32(want["sum"]))
    with pytest.raises(ValueError, match="mean"):
        cd.cumulative_rows(batch, ops=("sum", "mean"), sum_dtype=torch.int32)
    for bad in ((), ("median",), ("min", "range")):
        with pytest.raises(ValueError):
            cd.cumulative_rows(batch, ops=bad)
    with pytest.raises(ValueError):
        cd.cumulative_rows(batch, sum_dtype=torch.float32)
    with pytest.raises(ValueError):
        cd.cumulative_rows(batch, carry=carry.table)
    # three batches chained: the cumulative of the concatenation, and the mean goes on counting rows
    rows = (2 * 40 + 13, 40, G - 3 * 40 - 13)
    carry, parts, lo = None, [], 0
    for r in rows:
        piece = x[lo * D:(lo + r) * D]
        _, b = make_batch(sz, oracle, codec, esz, D, chunk_len, piece, False)
        res, carry = cd.cumulative_rows(b, ops=("min", "max", "sum", "mean"), carry=carry, return_carry=True)
        parts.append(res)
        lo += r
        assert carry.rows == lo
    for k in ("sum", "mean"):
        assert torch.equal(torch.cat([p[k] for p in parts]), got[k]), k
    for k in ("min", "max"):
        assert torch.equal(torch.cat([p[k].view(view) for p in parts]), got[k].view(view)), k
    assert np.array_equal(carry.table.cpu().numpy().view(np.uint64), left)
