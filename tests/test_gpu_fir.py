"""GPU tests (-m gpu) of FIR rows (sprintz_mi355x_fir_rows, ChunkedCodec.fir_rows / shift_rows / lag_diff_rows / smooth_rows): a per-column tap
filter over the rows, straight from a compressed batch, every element at its own place as int32 or converted floats.

The expected value is always the numpy model (tests/fir_model.py) on the ORIGINAL input, compared exactly: integers as they are, floats as
bits.  There are no tolerances.  Every launch runs on a sentinel-filled output and rets with padding around them and on a dirty scratch with
sentinels around it, and asserts its kernel family (tests/dispatch.py) against the planner's answer for the shape (tests/plan_probe.cpp, asked
with q=19 rows=T out_esz=...)."""
import os
import zlib

import numpy as np
import pytest

import derive_model as dm
import fir_model as fm
import float_model as flm
import planner
import rolling_model as rm
from dispatch import ran
from drive_tables import FIRE_SHAPES as FIRE_TABLE
from drive_tables import ROWOP_CASES, ROWOP_IDS, fire_batch, rowop_batch
from fir_runner import CODEC_ID, assert_fir, check_refusals, run_fir
from fixtures import chunks_per_group, gpu_lib, no_fast, sz  # noqa: F401  (fixtures)
from harness import DTYPES
from rowdata import FLOAT_FAST_SHAPES as FAST_SHAPES, GENERIC_SHAPES, gen_data, lowdim, make_batch
from streams import OLD, options, truncated_batch

pytestmark = pytest.mark.gpu

Q_FIR = 19
# no history; one row; a history of exactly one block (T - 1 = 8); one that rounds up to the next block; several blocks; T - 1 = R
TAPS = [1, 2, 3, 9, 10, 17, 65, 68]
FLOATS = (flm.F32, flm.F16, flm.BF16)


@pytest.fixture(scope="module")
def plan():
    """the planner on a host compiler: -> f(**fields) -> the family's name"""
    planner.available(required=True)
    known = {}

    def ask(**fields):
        key = tuple(sorted((k, int(v)) for k, v in fields.items()))
        if key not in known:
            got = planner.ask("decode", q=Q_FIR, **fields)
            assert got.get("family") in ("dec_fast", "dec_generic"), got
            known[key] = got["family"]
        return known[key]
    return ask


def rotate(key, k):
    return zlib.crc32(key.encode()) % k


def named_chunk_len(D):
    """67 rows: four groups of 16 and a verbatim tail of 3 rows; T = 68 reaches exactly one chunk back"""
    return D * (16 * 4 + 3)


def check_case(plan, batch, codec, esz, D, chunk_len, n, x, taps, bias, fmt, prev, general, fam, cpg, shift=0, bad=(), want=None):
    """one launch on the planner's family, against the model; -> that family"""
    taps = fm.as_taps(taps, D)
    T = taps.shape[0]
    scale, offset = dm.form_params(D) if fmt != fm.I32 else (None, None)
    if want is None:
        want = fm.fir_rows(x, D, taps, bias, fmt, scale, offset, prev)
    osz = fm.OUT_BYTES[fmt]
    family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=batch.nchunks, codec=CODEC_ID[codec], rows=T, out_esz=osz, general=general, no_fast=fam,
                  chunks_per_group=cpg, out_lo=(shift * osz) % 16)
    assert family == ("dec_fast" if fm.fast_takes(esz, D, chunk_len, T, general, fam, (shift * osz) % 16, osz) else "dec_generic")
    with ran(only=[family], **{family: 1}):
        buf, rets = run_fir(batch, codec, esz, D, chunk_len, taps, bias, fmt, scale, offset, prev, general, shift)
    assert_fir(buf, rets, n, chunk_len, batch.nchunks, D, T, want, shift, (codec, esz, D, T, fmt, prev is not None, general, fam, cpg, shift, family), bad)
    return family


# ------------------------------------------------------------------ parity

@pytest.mark.parametrize("codec,esz,D", [(codec, esz, D) for codec in ("delta", "xff") for esz, D in FAST_SHAPES + GENERIC_SHAPES])
def test_fir_rows_parity_named_shapes(sz, oracle, no_fast, chunks_per_group, plan, codec, esz, D):
    """the sixteen shapes named for the planner, both codecs, both families (NO_FAST), 1 and 3 chunks a lane group -- decode_fast.h's chunk loop,
    where the ring restarts cold with every chunk -- with and without the general layout, all eight T as int32 with random signed taps that differ
    per column, `prev` given at every second T; the three float formats on one leg each T, in rotation; 5 - 8 chunks of 67 rows, a short last chunk
    of 5 rows (fewer than most T - 1) or one that ends mid-row"""
    key = f"fir{codec}{esz}{D}"
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    chunk_len = named_chunk_len(D)
    nchunks = 5 + D % 4
    last = 5 * D if rotate(key, 2) or D == 1 else 37 * D + max(1, D // 2)
    n = (nchunks - 1) * chunk_len + last
    x = gen_data(("walk", "uniform", "sparse")[rotate(key, 3)], rng, n, esz, D)
    batches = {False: make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)[1]}
    batches[True] = make_batch(sz, oracle, codec, esz, D, chunk_len, x, True)[1] if lowdim(esz, D) else batches[False]
    legs = [(general, fam, cpg) for general in (False, True) for fam in (0, 1) for cpg in (1, 3)]
    seen = set()
    for i, T in enumerate(TAPS):
        taps, bias = fm.random_taps(rng, T, D, esz)
        prev = rng.integers(0, 1 << (8 * esz), (T - 1, D)).astype(DTYPES[esz]) if i % 2 == 0 and T > 1 else None
        want = fm.fir_rows(x, D, taps, bias, fm.I32, None, None, prev)
        ffmt = FLOATS[(i + rotate(key, 3)) % 3]
        fleg = legs[(i + rotate(key, 8)) % 8]
        for general, fam, cpg in legs:
            no_fast(fam)
            chunks_per_group(cpg)
            seen.add(check_case(plan, batches[general], codec, esz, D, chunk_len, n, x, taps, bias, fm.I32, prev, general, fam, cpg, want=want))
            if (general, fam, cpg) == fleg:
                check_case(plan, batches[general], codec, esz, D, chunk_len, n, x, taps, bias, ffmt, prev, general, fam, cpg)
    assert ("dec_fast" in seen) == ((esz, D) in ((2, 8), (2, 16), (2, 24), (2, 64), (1, 16))) and "dec_generic" in seen
    chunks_per_group(1)
    no_fast(0)


@pytest.mark.parametrize("codec,esz,D,R", [("xff", 2, 8, 80), ("delta", 2, 16, 67), ("xff", 1, 32, 72), ("delta", 1, 64, 67), ("xff", 2, 40, 72), ("delta", 2, 32, 67),
                                           ("xff", 1, 48, 80)])
def test_fir_rows_on_every_fast_mapping(sz, oracle, chunks_per_group, plan, codec, esz, D, R):
    """decode_fast.h's one-column-a-lane mappings that the mode has -- 8, 16, 32 and 64 lanes a chunk at either width, full and partly filled
    groups -- in every format at T = 3, 10 and 17, on walks with flat spans (run blocks); an output off the 16-byte grid runs the generic kernel"""
    rng = np.random.default_rng(R * D + esz)
    chunk_len, nchunks = D * R, 5
    n = nchunks * chunk_len - 9 * D - D // 2
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    seen = set()
    for T in (3, 10, 17):
        taps, bias = fm.random_taps(rng, T, D, esz)
        for cpg in (1, 3):
            chunks_per_group(cpg)
            for fmt in fm.FORMATS if cpg == 1 else (fm.FORMATS[T % 4],):
                seen.add(check_case(plan, batch, codec, esz, D, chunk_len, n, x, taps, bias, fmt, None, False, 0, cpg))
    assert seen == {"dec_fast"}
    chunks_per_group(1)
    taps, bias = fm.random_taps(rng, 9, D, esz)
    for shift in (1, 2):
        assert check_case(plan, batch, codec, esz, D, chunk_len, n, x, taps, bias, fm.I32, None, False, 0, 1, shift) == "dec_generic"


# ------------------------------------------------------------------ seams

def seam_data(rng, esz, D, R, nchunks, rows):
    """chunk c's rows hover around a level of its own, and the levels jump between chunks: the rows behind a seam differ from what a chunk-local
    history gives by far more than the noise"""
    level = np.array([60 + 90 * (c % 2) + 3 * (c % 3) for c in range(nchunks)])
    v = level[np.arange(rows) // R][:, None] + rng.integers(-3, 4, size=(rows, D))
    return v.astype(DTYPES[esz])


@pytest.mark.parametrize("codec,esz,D,R,fam", [("xff", 2, 8, 67, 0), ("delta", 1, 16, 16, 0), ("delta", 2, 5, 13, 0), ("xff", 1, 80, 67, 0), ("delta", 2, 8, 67, 1)])
def test_fir_rows_seams(sz, oracle, no_fast, chunks_per_group, plan, codec, esz, D, R, fam):
    """a short last chunk of one row; one of a row and a partial one; one ending mid-chunk, mid-row; `prev` given and NULL; a call of one chunk with
    and without `prev`; a batch shorter than T - 1 rows.  The input is such that the seam pass changes every chunk's first T - 1 rows"""
    no_fast(fam)
    rng = np.random.default_rng(D + esz + R)
    chunk_len, nchunks = D * R, 6
    Ts = [t for t in (2, 9, 12) if t - 1 <= R] + [R + 1]
    for tail_elems in (D, D + max(1, D // 2), R // 2 * D + D - 1):
        rows = (nchunks - 1) * R + -(-tail_elems // D)
        x = seam_data(rng, esz, D, R, nchunks, rows).ravel()[:(nchunks - 1) * chunk_len + tail_elems]
        n = x.size
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        for T in Ts:
            taps, bias = fm.random_taps(rng, T, D, esz)
            prev = (seam_data(rng, esz, D, R, 1, T - 1).astype(np.int64) + 50).astype(DTYPES[esz])
            true, local = fm.sums(x, D, taps, bias), fm.sums_local(x, chunk_len, D, taps, bias)
            head = np.arange(n) % chunk_len // D < T - 1
            assert np.array_equal(true[~head], local[~head]) and (true[head] != local[head]).any()
            assert (fm.sums(x, D, taps, bias, prev)[:D] != true[:D]).any()
            for cpg in (1, 3):
                chunks_per_group(cpg)
                for fmt, pv in ((fm.I32, None), (fm.I32, prev), (flm.F32, prev), (flm.BF16, None)):
                    check_case(plan, batch, codec, esz, D, chunk_len, n, x, taps, bias, fmt, pv, False, fam, cpg)
    chunks_per_group(1)
    # one chunk, and batches shorter than T - 1 rows (of 1 row, and of T - 2 rows and a partial one)
    T = Ts[-2]
    taps, bias = fm.random_taps(rng, T, D, esz)
    prev = rng.integers(0, 1 << (8 * esz), (T - 1, D)).astype(DTYPES[esz])
    for x1 in (x[:chunk_len - D - 1], x[:D], x[:(T - 2) * D + D // 2] if T > 2 else x[:D]):
        cd, one = make_batch(sz, oracle, codec, esz, D, chunk_len, x1, False)
        for pv in (None, prev):
            check_case(plan, one, codec, esz, D, chunk_len, x1.size, x1, taps, bias, fm.I32, pv, False, fam, 1)
            check_case(plan, one, codec, esz, D, chunk_len, x1.size, x1, taps, bias, flm.F16, pv, False, fam, 1)
    no_fast(0)


@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 5), ("delta", 2, 80)])
def test_fir_rows_stream_cut_into_two_batches(sz, oracle, codec, esz, D):
    """a stream cut at a row that is no chunk boundary: the second call takes the first's return_tail, and the two results joined equal the one-batch
    result -- with and without a prev in front of the first; a first batch shorter than T - 1 rows hands its prev on"""
    import torch
    rng = np.random.default_rng(7 * D + esz)
    chunk_len = D * 67
    G = 4 * 67 + 29
    x = gen_data("walk", rng, G * D, esz, D)
    dev = lambda a: torch.from_numpy(a.view(np.int8 if esz == 1 else np.int16)).cuda()      # noqa: E731
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device="cuda:0")
    whole = cd.compress(dev(x).view(cd.dtype))
    for T in (2, 9, 17, 68):
        taps, bias = fm.random_taps(rng, T, D, esz)
        prev = rng.integers(0, 1 << (8 * esz), (T - 1, D)).astype(DTYPES[esz])
        for cut in (2 * 67 + 11, 3):                                               # mid-chunk; fewer rows than most T - 1
            a, b = cd.compress(dev(x[:cut * D]).view(cd.dtype)), cd.compress(dev(x[cut * D:]).view(cd.dtype))
            for pv in (None, prev):
                pt = None if pv is None else dev(pv).view(cd.dtype)
                one = cd.fir_rows(whole, taps.tolist(), bias.tolist(), prev=pt)
                assert np.array_equal(one.cpu().numpy().reshape(-1).astype(np.int64), fm.sums(x, D, taps, bias, pv))
                ya, tail = cd.fir_rows(a, taps.tolist(), bias.tolist(), prev=pt, return_tail=True)
                assert tail.shape == (T - 1, D) and tail.dtype == cd.dtype
                assert np.array_equal(tail.cpu().view(torch.int8 if esz == 1 else torch.int16).numpy().view(DTYPES[esz]), fm.tail_rows(x[:cut * D], D, T, pv))
                yb, tail2 = cd.fir_rows(b, taps.tolist(), bias.tolist(), prev=tail, return_tail=True)
                assert torch.equal(torch.cat([ya, yb]), one)
                assert np.array_equal(tail2.cpu().view(torch.int8 if esz == 1 else torch.int16).numpy().view(DTYPES[esz]), x.reshape(G, D)[G - (T - 1):])


# ------------------------------------------------------------------ the two drives

@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_fir_rows_over_runs(sz, oracle, no_fast, chunks_per_group, plan, codec, w, D, kind):
    """tests/rle_drive.py's batches: runs of 1 .. 16 blocks and maximal ones, at chunk starts and ending at the chunk's last block -- runs enter,
    cross and leave a block while the ring is warm and cold; on the planner's family at 1 and 3 chunks a lane group and on the generic kernel"""
    cd, batch, data, chunk_len, _ = rowop_batch(sz, oracle, codec, w, D, kind)
    esz = w // 8
    rng = np.random.default_rng(w + D)
    with options(**OLD):
        for T in (9, 17):
            taps, bias = fm.random_taps(rng, T, D, esz)
            want = fm.fir_rows(data, D, taps, bias)
            for fam, cpgs in ((0, (1, 3)), (1, (1,))):
                no_fast(fam)
                for cpg in cpgs:
                    chunks_per_group(cpg)
                    check_case(plan, batch, codec, esz, D, chunk_len, data.size, data, taps, bias, fm.I32, None, False, fam, cpg, want=want)
            check_case(plan, batch, codec, esz, D, chunk_len, data.size, data, taps, bias, flm.F32 if T == 9 else flm.BF16, None, False, 1, 1)
    chunks_per_group(1)
    no_fast(0)


@pytest.mark.parametrize("w,D", list(FIRE_TABLE), ids=[f"u{w}x{D}" for w, D in FIRE_TABLE])
def test_fir_rows_on_the_fire_drive(sz, oracle, chunks_per_group, plan, w, D):
    """tests/fire_drive.py's batches: FIRE counters through their int16 wrap, runs replayed at frozen extreme coefficients"""
    cd, batch, data, chunk_len, nchunks = fire_batch(sz, oracle, w, D)
    rng = np.random.default_rng(w * D)
    with options(**OLD):
        for T in (9, 17):
            taps, bias = fm.random_taps(rng, T, D, w // 8)
            want = fm.fir_rows(data, D, taps, bias)
            for cpg in (1, 3):
                chunks_per_group(cpg)
                check_case(plan, batch, "xff", w // 8, D, chunk_len, data.size, data, taps, bias, fm.I32, None, False, 0, cpg, want=want)
    chunks_per_group(1)


# ------------------------------------------------------------------ wrap

@pytest.mark.parametrize("codec,esz,D,fam", [("xff", 2, 8, 0), ("delta", 1, 5, 0), ("delta", 2, 8, 1), ("xff", 1, 80, 0)])
def test_fir_rows_wraps_as_the_header_says(sz, oracle, no_fast, plan, codec, esz, D, fam):
    """the C entry point with taps the Python layer refuses (anywhere in int32): the sums wrap modulo 2^32, exactly as the model's do"""
    no_fast(fam)
    rng = np.random.default_rng(D + esz + fam)
    chunk_len, nchunks = D * 67, 4
    n = nchunks * chunk_len - 20 * D
    x = gen_data("uniform", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    for T in (2, 10):
        taps, bias = fm.random_taps(rng, T, D, esz, exact=False)
        taps[0, 0], taps[T - 1, D - 1], bias[0] = -(1 << 31), (1 << 31) - 1, -(1 << 31)      # the int32 limits themselves
        assert min(fm.bound(esz, taps, bias, D)) > 1 << 31
        for fmt in (fm.I32, flm.F32):
            check_case(plan, batch, codec, esz, D, chunk_len, n, x, taps, bias, fmt, None, False, fam, 1)
    with pytest.raises(ValueError, match="column 0's filter can reach"):
        cd.fir_rows(batch, [(1 << 31) - 1, 1])
    no_fast(0)


# ------------------------------------------------------------------ damage

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 32), ("delta", 2, 12), ("xff", 1, 80)])
def test_fir_rows_damaged_chunk(sz, oracle, chunks_per_group, plan, codec, esz, D):
    """one truncated chunk in the middle: its rets entry is negative and every other chunk's is its count (decompress_batch's); every row outside the
    damaged chunk and outside the first T - 1 rows behind it is exact; the sentinels around the output and the scratch stand; check=True names the chunk"""
    import torch
    rng = np.random.default_rng(3 * D)
    chunk_len, nchunks, cut = D * 67, 7, 3
    n = nchunks * chunk_len - 5 * D
    x = seam_data(rng, esz, D, 67, nchunks, n // D).ravel()
    cd, good = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    batch = truncated_batch(sz, good, cut)
    with options(**OLD):
        plain_rets = torch.full((nchunks,), -77, dtype=torch.int64, device="cuda")
        cd.decompress(batch, rets=plain_rets)
        plain_rets = plain_rets.cpu().numpy()
        assert plain_rets[cut] < 0 and np.all(np.delete(plain_rets, cut) > 0)
        for cpg in (3, 1):
            chunks_per_group(cpg)
            for T, fmt in ((1, fm.I32), (3, fm.I32), (17, flm.F32), (68, fm.I32)):
                taps, bias = fm.random_taps(rng, T, D, esz)
                check_case(plan, batch, codec, esz, D, chunk_len, n, x, taps, bias, fmt, None, False, 0, cpg, bad=(cut,))
        with pytest.raises(sz.SprintzError, match=f"fir_rows: chunk {cut} "):
            cd.fir_rows(batch, [1, -1])
        with pytest.raises(sz.SprintzError, match=f"fir_rows: chunk {cut} "):
            cd.lag_diff_rows(batch, 2)
        got = cd.fir_rows(batch, [1, 2, 1], check=False)
        assert got.shape == (n // D, D)
        cd.fir_rows(good, [1, 2, 1])                                               # undamaged: no error
    chunks_per_group(1)


# ------------------------------------------------------------------ what the library already computes

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 5), ("delta", 2, 80), ("xff", 1, 16)])
def test_fir_rows_meets_rolling_diff_and_decompress(sz, oracle, codec, esz, D):
    """taps of W ones with a prev of zeros equal rolling_rows' sum; lag_diff_rows(batch, 1) equals diff_rows; shift_rows(batch, k) equals the
    decoded tensor moved by k rows with the first k rows replicated; a second difference and smooth_rows against torch on decompress' output"""
    import torch
    rng = np.random.default_rng(13 * D + esz)
    chunk_len = D * 67
    G = 5 * 67 + 20
    x = gen_data("walk", rng, G * D, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    flat = cd.decompress(batch).reshape(-1).view(torch.int8 if esz == 1 else torch.int16).cpu().numpy().view(DTYPES[esz])
    assert np.array_equal(flat, x)
    v = torch.from_numpy(x.astype(np.int32)).cuda().view(G, D)
    for W in (8, 16, 64):
        zeros = torch.zeros((W - 1, D), dtype=torch.int16 if esz == 2 else torch.int8, device="cuda").view(cd.dtype)
        assert torch.equal(cd.fir_rows(batch, [1] * W, prev=zeros), cd.rolling_rows(batch, W, ops=("sum",))["sum"])
    if D <= 16:
        assert torch.equal(cd.lag_diff_rows(batch, 1), cd.diff_rows(batch))
    else:
        cols = [0, D // 2, D - 1]
        assert torch.equal(cd.lag_diff_rows(batch, 1)[:, cols], cd.diff_rows(batch, cols))
    for k in (0, 1, 7, 8, 30, 67):
        moved = torch.cat([v[:1].expand(k, D), v[:G - k]]) if k else v
        assert torch.equal(cd.shift_rows(batch, k), moved), k
    for p in (2, 24):
        assert torch.equal(cd.lag_diff_rows(batch, p)[p:], v[p:] - v[:-p])
        assert torch.equal(cd.lag_diff_rows(batch, p)[:p], v[:p] - v[:1])
    second = cd.fir_rows(batch, [1, -2, 1])
    assert torch.equal(second[2:], v[2:] - 2 * v[1:-1] + v[:-2])
    sm = cd.smooth_rows(batch, [1, 2, 3, 2, 1])
    pad = torch.cat([v[:1].expand(4, D), v]).cpu()
    s = sum(c * pad[4 - j:4 - j + G] for j, c in enumerate([1, 2, 3, 2, 1]))
    want = (s.to(torch.float32) * torch.tensor(1.0 / 9, dtype=torch.float32)).to(torch.float32)
    assert sm.dtype == torch.float32 and torch.equal(sm.cpu().view(torch.int32), want.view(torch.int32))
    for name, call in (("shift_rows", lambda: cd.shift_rows(batch, 1, taps=[1])), ("lag_diff_rows", lambda: cd.lag_diff_rows(batch, 1, taps=[1]))):
        with pytest.raises(ValueError, match=f"{name} builds taps itself"):
            call()
    with pytest.raises(ValueError, match="smooth_rows builds scale itself"):
        cd.smooth_rows(batch, [1, 1], scale=0.5)
    for bad in ([[1] * D, [2] * D], torch.ones((2, D), dtype=torch.int32), 3):      # per-column taps have no one sum to scale by
        with pytest.raises(ValueError, match="smooth_rows takes 1-D taps"):
            cd.smooth_rows(batch, bad)


# ------------------------------------------------------------------ float formats and Python

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 5), ("delta", 2, 80)])
def test_fir_rows_python(sz, oracle, plan, codec, esz, D):
    """fir_rows against the torch expression on decompress' output, bit for bit in every float format, with sums above 2^24; a batch that ends
    mid-row returns the flat view; out= reuse, rets=, a side stream, the refusals"""
    import torch
    rng = np.random.default_rng(11 * D)
    chunk_len = D * 67
    n = 4 * chunk_len + 20 * D
    x = gen_data("uniform", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    G = n // D
    v = torch.from_numpy(x.astype(np.int64)).view(G, D)
    taps, bias = fm.random_taps(rng, 5, D, esz)
    tt, tb = torch.from_numpy(taps), torch.from_numpy(bias)
    pad = torch.cat([v[:1].expand(4, D), v])
    s = sum(tt[j] * pad[4 - j:4 - j + G] for j in range(5)) + tb
    assert s.abs().max() > 1 << 24 and s.abs().max() < 1 << 31
    family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=batch.nchunks, codec=CODEC_ID[codec], rows=5, out_esz=4)
    with ran(only=[family], **{family: 1}):
        got = cd.fir_rows(batch, taps.tolist(), bias.tolist())
    assert got.shape == (G, D) and got.dtype == torch.int32 and got.device.type == "cuda" and got.is_contiguous()
    assert torch.equal(got.cpu(), s.to(torch.int32))
    assert torch.equal(cd.fir_rows(batch, torch.from_numpy(taps).cuda(), bias.tolist(), general_layout=True), got)
    scale, offset = dm.form_params(D)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        f = cd.fir_rows(batch, taps.tolist(), bias.tolist(), dtype=dtype, scale=scale.tolist(), offset=torch.from_numpy(offset))
        want = (s.to(torch.int32).to(torch.float32) * torch.from_numpy(scale) + torch.from_numpy(offset)).to(dtype)
        assert f.dtype == dtype and f.shape == (G, D)
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(f.cpu().view(bits), want.view(bits))
    # a batch that ends mid-row: the flat view of its elements
    cut = x[:n - D - 2]
    cdc, ragged = make_batch(sz, oracle, codec, esz, D, chunk_len, cut, False)
    flat = cdc.fir_rows(ragged, taps.tolist(), bias.tolist())
    assert flat.shape == (cut.size,) and np.array_equal(flat.cpu().numpy().astype(np.int64), fm.sums(cut, D, taps, bias))
    # out=: written in place; rets=; too small, of the wrong dtype or not contiguous is refused
    slot = batch.nchunks * chunk_len
    out = torch.zeros(slot + 7, dtype=torch.int32, device="cuda")
    res = cd.fir_rows(batch, taps.tolist(), bias.tolist(), out=out)
    assert res.data_ptr() == out.data_ptr() and torch.equal(res, got)
    rets = torch.full((batch.nchunks,), -1, dtype=torch.int64, device="cuda")
    cd.fir_rows(batch, [1], rets=rets)
    assert rets.tolist() == [min(chunk_len, n - c * chunk_len) for c in range(batch.nchunks)]
    for bad in (torch.zeros(slot - 1, dtype=torch.int32, device="cuda"), torch.zeros(slot, dtype=torch.float32, device="cuda"),
                torch.zeros(slot * 2, dtype=torch.int32, device="cuda")[::2], torch.zeros(slot, dtype=torch.int32), np.zeros(slot)):
        with pytest.raises(ValueError):
            cd.fir_rows(batch, [1, 2], out=bad)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = cd.fir_rows(batch, taps.tolist(), bias.tolist())
    side.synchronize()
    assert torch.equal(on_side, got)
    for kw in (dict(scale=2.0), dict(offset=1.0)):                                  # a float dtype alone takes them
        with pytest.raises(ValueError):
            cd.fir_rows(batch, [1], **kw)
    with pytest.raises(ValueError):
        cd.fir_rows(batch, [1, 2], dtype=torch.float32, scale=[1.0] * (D + 1))
    with pytest.raises(ValueError):
        cd.fir_rows(batch, [1], dtype=torch.float64)
    with pytest.raises(ValueError):
        cd.fir_rows(batch, [1] * 257)
    with pytest.raises(ValueError, match="more than the 67 rows of a chunk"):
        cd.fir_rows(batch, [1] * 69)
    with pytest.raises(ValueError):
        cd.fir_rows(batch, [1, 1], prev=[0] * (D + 1))
    with pytest.raises(ValueError):
        sz.ChunkedCodec(codec, esz, D, chunk_len + 1, device="cuda:0").fir_rows(batch, [1])      # chunk_len % ndims != 0


def test_fir_rows_no_chunks_and_refusals(sz, gpu_lib):
    """nchunks == 0 returns 0 and launches nothing; every refusal of the header comes back with its code and names the operation, on device pointers
    as on host pointers, and launches nothing either"""
    import torch
    mem = torch.full((16384 + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    p = (mem.data_ptr() + 15) & ~15
    with ran(only=[]):
        check_refusals(gpu_lib, p)
    torch.cuda.synchronize()
    assert torch.all(mem == 0x5A)


# ------------------------------------------------------------------ the headline geometry

def test_fir_rows_at_the_headline_geometry(sz, oracle, plan):
    """uint16 x 8, FIRE, 10 KB chunks, T = 65, chunks_per_group as the library defaults: the real chunk size, the real ring budget and a
    workgroup's last partial group (389 chunks); a short last chunk"""
    import torch
    esz, D, chunk_len, nchunks, T = 2, 8, 5120, 389, 65
    rng = np.random.default_rng(65)
    n = nchunks * chunk_len - 37 * D
    x = gen_data("walk", rng, n, esz, D)
    cd = sz.ChunkedCodec("xff", esz, D, chunk_len, device="cuda:0")
    batch = cd.compress(torch.from_numpy(x.view(np.int16)).cuda().view(cd.dtype))
    taps, bias = fm.random_taps(rng, T, D, esz)
    family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=1, rows=T, out_esz=4, chunks_per_group=int(os.environ.get("SPRINTZ_MI355X_CHUNKS_PER_GROUP", 1)))
    assert family == "dec_fast"
    for fmt in (fm.I32, flm.F32):
        scale, offset = dm.form_params(D) if fmt != fm.I32 else (None, None)
        with ran(only=[family], **{family: 1}):
            buf, rets = run_fir(batch, "xff", esz, D, chunk_len, taps, bias, fmt, scale, offset)
        assert_fir(buf, rets, n, chunk_len, nchunks, D, T, fm.fir_rows(x, D, taps, bias, fmt, scale, offset), 0, ("headline", fmt))
