"""GPU tests (-m gpu) of derive rows (sprintz_mi355x_derive_rows, ChunkedCodec.derive_rows / diff_rows): K linear forms of every row and the row
in front of it, straight from a compressed batch into a dense [G, K] tensor of int32 or converted floats.

The expected value is always the numpy model (tests/derive_model.py) on the ORIGINAL input, compared exactly: integers as they are, floats as
bits.  There are no tolerances.  Every launch runs on a sentinel-filled output and rets with padding around them and on a dirty scratch, and
asserts its kernel family (tests/dispatch.py) against the planner's answer for the shape (tests/plan_probe.cpp, asked with q=18 rows=K
out_esz=...)."""
import zlib

import numpy as np
import pytest

import derive_model as dm
import float_model as fm
import linear_model as lm
import planner
from derive_runner import CODEC_ID, PAD, assert_derive, check_refusals, run_derive
from dispatch import ran
from drive_tables import FIRE_SHAPES as FIRE_TABLE
from drive_tables import ROWOP_CASES, ROWOP_IDS, fire_batch, rowop_batch
from fixtures import chunks_per_group, gpu_lib, no_fast, sz  # noqa: F401  (fixtures)
from harness import DTYPES
from rowdata import DATA, gen_data, lowdim, make_batch, quartiles, weight_sets
from streams import OLD, options, truncated_batch

pytestmark = pytest.mark.gpu

Q_DERIVE = 18
NDIMS = [1, 2, 3, 5, 8, 16, 33, 64, 65, 80, 128, 300]
KS = [1, 2, 3, 8, 16]
ROWS = [67, 16, 13]                                    # four groups and a 3-row verbatim tail; one group; fewer than 16: all tail


@pytest.fixture(scope="module")
def plan():
    """the planner on a host compiler: -> f(**fields) -> the family's name"""
    planner.available(required=True)
    known = {}

    def ask(**fields):
        key = tuple(sorted((k, int(v)) for k, v in fields.items()))
        if key not in known:                               # (one probe process a distinct question)
            got = planner.ask("decode", q=Q_DERIVE, **fields)
            assert got.get("family") in ("dec_fast", "dec_generic"), got
            known[key] = got["family"]
        return known[key]
    return ask


def rotate(key, k):
    return zlib.crc32(key.encode()) % k


def stacked_forms(rng, x, esz, D, lag, K, rot):
    """rowdata.weight_sets' single / a - b / ones / random (the random one at B = 2^31 - 1), stacked into K forms from set `rot` on"""
    sets = weight_sets(rng, x, esz, D, lag)[:4]
    order = [sets[(rot + k) % 4] for k in range(K)]
    w = np.stack([np.asarray(s[1], np.int64) for s in order])
    u = np.stack([np.asarray(s[2], np.int64) for s in order]) if lag else None
    bias = np.array([s[3] for s in order], np.int64)
    return w, u, bias


def check_case(plan, batch, codec, esz, D, chunk_len, n, x, w, u, bias, fmt, prev, general, fam, cpg, shift=0, bad=()):
    """one launch on the planner's family, against the model; -> that family"""
    K = w.shape[0]
    scale, offset = dm.form_params(K) if fmt != dm.I32 else (None, None)
    want = dm.derive_rows(x, D, w, u, bias, fmt, scale, offset, prev)
    osz = dm.OUT_BYTES[fmt]
    family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=batch.nchunks, codec=CODEC_ID[codec], rows=K, out_esz=osz, general=general, no_fast=fam,
                  chunks_per_group=cpg, out_lo=(shift * osz) % 16)
    assert family == ("dec_fast" if dm.fast_takes(esz, D, chunk_len, K, osz, general, fam, (shift * osz) % 16) else "dec_generic")
    with ran(only=[family], **{family: 1}):
        buf, rets = run_derive(batch, codec, esz, D, chunk_len, w, u, bias, fmt, scale, offset, prev, general, shift)
    assert_derive(buf, rets, n, chunk_len, batch.nchunks, D, K, want, shift, (codec, esz, D, K, fmt, u is not None, prev is not None, general, fam, cpg, shift, family),
                  bad, u is not None)
    return family


# ------------------------------------------------------------------ parity

def parity_schedule(codec, esz, D):
    """-> (rows a chunk, chunks, data, [(general, NO_FAST, chunks a group, lag, K, format, prev given)]): the axes rotated over the cases"""
    j = NDIMS.index(D)
    c = (1 if codec == "xff" else 0) + 2 * (esz - 1)
    R = ROWS[(j + c) % 3]
    nchunks = 3 + (j + c) % 5
    data = DATA[(j + c) % 4]
    legs = [(False, 0, 1), (False, 0, 3), (False, 1, 1)] + ([(True, 0, 1), (True, 1, 1)] if lowdim(esz, D) else [])
    runs = []
    i = j + 5 * c
    for general, fam, cpg in legs:
        for lag in (False, True):
            runs.append((general, fam, cpg, lag, KS[i % 5], dm.FORMATS[(i // 2 + lag) % 4], lag and i % 3 != 0))
            i += 1
    return R, nchunks, data, runs


PARITY = [(codec, esz, D) for codec in ("delta", "xff") for esz in (1, 2) for D in NDIMS]


def test_parity_schedule_meets_every_triple():
    """both families in all four formats with and without a lag term; every K with and without; every ndims on both codecs and widths"""
    triples, ks = set(), set()
    for codec, esz, D in PARITY:
        R, _, _, runs = parity_schedule(codec, esz, D)
        for general, fam, cpg, lag, K, fmt, _ in runs:
            fast = dm.fast_takes(esz, D, D * R, K, dm.OUT_BYTES[fmt], general, fam, 0)
            triples.add((fast, fmt, lag))
            ks.add((K, lag))
    assert triples == {(f, fmt, lag) for f in (False, True) for fmt in dm.FORMATS for lag in (False, True)}
    assert ks == {(K, lag) for K in KS for lag in (False, True)}


@pytest.mark.parametrize("codec,esz,D", PARITY)
def test_derive_rows_parity(sz, oracle, no_fast, chunks_per_group, plan, codec, esz, D):
    """both codecs, both widths, twelve ndims; chunks of 67, 16 and 13 rows, 3 to 7 of them, the last one short and ending mid-row; walk, uniform,
    constant and sparse data; 1 and 3 chunks a lane group, the generic kernel under NO_FAST, the general layout on the low-dim shapes; K, the
    format, the lag term and `prev` rotated (parity_schedule); the random form sits at B = 2^31 - 1"""
    key = f"derive{codec}{esz}{D}"
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    R, nchunks, data, runs = parity_schedule(codec, esz, D)
    chunk_len = D * R
    n = (nchunks - 1) * chunk_len + (R // 3 + 1) * D + D // 2          # a short last chunk that ends mid-row (D > 1)
    x = gen_data(data, rng, n, esz, D)
    batches = {False: make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)}
    if lowdim(esz, D):
        batches[True] = make_batch(sz, oracle, codec, esz, D, chunk_len, x, True)
    top = (1 << (8 * esz)) - 1
    for r, (general, fam, cpg, lag, K, fmt, with_prev) in enumerate(runs):
        cd, batch = batches[general]
        no_fast(fam)
        chunks_per_group(cpg)
        w, u, bias = stacked_forms(rng, x, esz, D, lag, K, r)
        prev = rng.integers(0, top + 1, D).astype(DTYPES[esz]) if with_prev else None
        check_case(plan, batch, codec, esz, D, chunk_len, n, x, w, u, bias, fmt, prev, general, fam, cpg)
    chunks_per_group(1)
    no_fast(0)


@pytest.mark.parametrize("codec,esz,D,R", [("xff", 2, 8, 80), ("delta", 2, 4, 80), ("xff", 1, 6, 80), ("delta", 1, 8, 80), ("xff", 1, 64, 72), ("delta", 2, 33, 80),
                                           ("xff", 2, 40, 72), ("delta", 1, 32, 67), ("xff", 2, 16, 67)])
def test_derive_rows_on_every_fast_mapping(sz, oracle, chunks_per_group, plan, codec, esz, D, R):
    """decode_fast.h's one-column-a-lane mappings -- 4, 8, 16, 32 and 64 lanes a chunk at either width, full and partly filled groups -- at every K
    in every format, with a lag term: the derived block smaller than, equal to and larger than the decoded one (the staging the launch asks for), an
    output off the 16-byte grid on the generic kernel; walks with flat spans (run blocks)"""
    rng = np.random.default_rng(R * D + esz)
    chunk_len, nchunks = D * R, 5
    n = nchunks * chunk_len - 9 * D - D // 2
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    seen = set()
    for i, K in enumerate(KS):
        for cpg in (1, 3):
            chunks_per_group(cpg)
            for fmt in dm.FORMATS if cpg == 1 else (dm.FORMATS[i % 4],):
                w, u, bias = stacked_forms(rng, x, esz, D, True, K, i)
                seen.add(check_case(plan, batch, codec, esz, D, chunk_len, n, x, w, u, bias, fmt, None, False, 0, cpg))
    assert seen == {"dec_fast"}
    chunks_per_group(1)
    w, u, bias = stacked_forms(rng, x, esz, D, True, 3, 0)
    for shift in (1, 2):
        assert check_case(plan, batch, codec, esz, D, chunk_len, n, x, w, u, bias, dm.I32, None, False, 0, 1, shift) == "dec_generic"


# ------------------------------------------------------------------ wrap

@pytest.mark.parametrize("codec,esz,D,fam", [("xff", 2, 8, 0), ("delta", 1, 5, 0), ("delta", 2, 8, 1), ("xff", 1, 80, 0)])
def test_derive_rows_wraps_as_the_header_says(sz, oracle, no_fast, plan, codec, esz, D, fam):
    """the C entry point with forms the Python layer refuses (B > 2^31): the sums wrap modulo 2^32, exactly as the model's do"""
    no_fast(fam)
    rng = np.random.default_rng(D + esz + fam)
    chunk_len, nchunks = D * 67, 4
    n = nchunks * chunk_len - 20 * D
    x = gen_data("uniform", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    for lag in (False, True):
        w = rng.integers(lm.INT32_MIN, lm.INT32_MAX + 1, (2, D))
        u = rng.integers(lm.INT32_MIN, lm.INT32_MAX + 1, (2, D)) if lag else None
        bias = rng.integers(lm.INT32_MIN, lm.INT32_MAX + 1, 2)
        for k in range(2):
            assert lm.bound_B(esz, w[k], None if u is None else u[k], bias[k]) > 1 << 31
        for fmt in (dm.I32, fm.F32):
            check_case(plan, batch, codec, esz, D, chunk_len, n, x, w, u, bias, fmt, None, False, fam, 1)
    with pytest.raises(ValueError, match="form 0 can reach"):
        cd.derive_rows(batch, [lm.INT32_MAX])
    no_fast(0)


# ------------------------------------------------------------------ seams

def seam_data(rng, esz, D, R, nchunks, rows):
    """chunk c's rows hover around a level of its own, and the levels jump between chunks: a chunk's first row differs from its TRUE predecessor by
    far more than from itself"""
    level = np.array([60 + 90 * (c % 2) + 3 * (c % 3) for c in range(nchunks)])
    v = level[np.arange(rows) // R][:, None] + rng.integers(-3, 4, size=(rows, D))
    return v.astype(DTYPES[esz])


@pytest.mark.parametrize("codec,esz,D,R,fam", [("xff", 2, 8, 67, 0), ("delta", 1, 16, 16, 0), ("delta", 2, 5, 13, 0), ("xff", 1, 80, 67, 0), ("delta", 2, 8, 67, 1)])
def test_derive_rows_seams(sz, oracle, no_fast, chunks_per_group, plan, codec, esz, D, R, fam):
    """a short last chunk of one row; a last chunk ending mid-row (its K places keep the sentinel: assert_derive); `prev` given and NULL; a call of
    one chunk with `prev`.  The input is such that the result differs from the self_rows model at every chunk's first row: what the seam pass is for"""
    no_fast(fam)
    rng = np.random.default_rng(D + esz + R)
    chunk_len, nchunks = D * R, 6
    e = np.eye(D, dtype=np.int64)
    w = np.stack([e[D // 2], e[0] - e[D - 1], np.ones(D, np.int64)])
    u = np.stack([-e[D // 2], e[D - 1], -np.ones(D, np.int64)])
    bias = np.array([0, 7, -3], np.int64)
    for tail_elems in (D, D + max(1, D // 2), R // 2 * D + D - 1):        # one row; one row and a partial one; mid-chunk, mid-row
        rows = (nchunks - 1) * R + -(-tail_elems // D)
        x = seam_data(rng, esz, D, R, nchunks, rows).ravel()[:(nchunks - 1) * chunk_len + tail_elems]
        n = x.size
        starts = tuple(range(0, n // D, R))
        true, selfed = dm.sums(x, D, w, u, bias), dm.sums(x, D, w, u, bias, self_rows=starts)
        assert all((true[g] != selfed[g]).any() for g in starts[1:]) and np.array_equal(np.delete(true, starts, 0), np.delete(selfed, starts, 0))
        prev = (x[:D].astype(np.int64) + 50).astype(DTYPES[esz])
        assert (dm.sums(x, D, w, u, bias, prev=prev)[0] != true[0]).any()
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        for cpg in (1, 3):
            chunks_per_group(cpg)
            for fmt, pv in ((dm.I32, None), (dm.I32, prev), (fm.F32, prev), (fm.BF16, None)):
                check_case(plan, batch, codec, esz, D, chunk_len, n, x, w, u, bias, fmt, pv, False, fam, cpg)
            check_case(plan, batch, codec, esz, D, chunk_len, n, x, w, None, bias, dm.I32, prev, False, fam, cpg)      # no lag term: prev is ignored
    chunks_per_group(1)
    # one chunk: without prev no seam pass runs, with prev it does
    x1 = x[:chunk_len - D - 1]
    cd, one = make_batch(sz, oracle, codec, esz, D, chunk_len, x1, False)
    for pv in (None, prev):
        check_case(plan, one, codec, esz, D, chunk_len, x1.size, x1, w, u, bias, dm.I32, pv, False, fam, 1)
        check_case(plan, one, codec, esz, D, chunk_len, x1.size, x1, w, u, bias, fm.F16, pv, False, fam, 1)
    no_fast(0)


# ------------------------------------------------------------------ damage

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 32), ("delta", 2, 12), ("xff", 1, 80)])
def test_derive_rows_damaged_chunk(sz, oracle, chunks_per_group, plan, codec, esz, D):
    """one truncated chunk in the middle: its rets entry is negative and every other chunk's is its count (decompress_batch's); every row of the
    other chunks is exact but, with a lag term, row 0 of the chunk behind it; the sentinels around the output stand; check=True names the chunk"""
    import torch
    rng = np.random.default_rng(3 * D)
    chunk_len, nchunks, cut = D * 67, 7, 3
    n = nchunks * chunk_len - 5 * D
    x = seam_data(rng, esz, D, 67, nchunks, n // D).ravel()
    cd, good = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    batch = truncated_batch(sz, good, cut)
    with options(**OLD):
        chunks_per_group(3)
        plain_rets = torch.full((nchunks,), -77, dtype=torch.int64, device="cuda")
        cd.decompress(batch, rets=plain_rets)
        plain_rets = plain_rets.cpu().numpy()
        assert plain_rets[cut] < 0 and np.all(np.delete(plain_rets, cut) > 0)
        for lag in (False, True):
            for K, fmt in ((3, dm.I32), (2, fm.F32)):
                w, u, bias = stacked_forms(rng, x, esz, D, lag, K, 1)
                check_case(plan, batch, codec, esz, D, chunk_len, n, x, w, u, bias, fmt, None, False, 0, 3, bad=(cut,))
        with pytest.raises(sz.SprintzError, match=f"derive_rows: chunk {cut} "):
            cd.derive_rows(batch, [{0: 1}], lag_forms=[{0: -1}])
        with pytest.raises(sz.SprintzError, match=f"derive_rows: chunk {cut} "):
            cd.diff_rows(batch, [0])
        got = cd.derive_rows(batch, [{0: 1}, 1], check=False)
        assert got.shape == (n // D, 2)
        cd.derive_rows(good, [{0: 1}])                                             # undamaged: no error
    chunks_per_group(1)


# ------------------------------------------------------------------ the two drives

def drive_forms(D, lag):
    e = np.eye(D, dtype=np.int64)
    w = np.stack([e[D - 1], np.ones(D, np.int64), e[0] - e[D - 1] if D > 1 else e[0]])
    u = np.stack([-e[D - 1], np.ones(D, np.int64), np.zeros(D, np.int64)]) if lag else None      # w + u = 0, w + u != 0, no lag in one form
    return w, u, np.array([0, -5, 9], np.int64)


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_derive_rows_over_runs(sz, oracle, no_fast, chunks_per_group, plan, codec, w, D, kind):
    """tests/rle_drive.py's batches: runs of 1 .. 16 blocks and maximal ones, at chunk starts and ending at the chunk's last block -- the run
    blocks' values, the lag term over a run's edges and the cursor's advance; on the planner's family at 1 and 3 chunks a lane group and on the
    generic kernel"""
    cd, batch, data, chunk_len, _ = rowop_batch(sz, oracle, codec, w, D, kind)
    esz = w // 8
    with options(**OLD):
        for fam, cpgs in ((0, (1, 3)), (1, (1,))):
            no_fast(fam)
            for cpg in cpgs:
                chunks_per_group(cpg)
                for lag in (False, True):
                    fw, fu, fb = drive_forms(D, lag)
                    for fmt in ((dm.I32, fm.BF16) if cpg == 1 else (fm.F32,)):
                        check_case(plan, batch, codec, esz, D, chunk_len, data.size, data, fw, fu, fb, fmt, None, False, fam, cpg)
    chunks_per_group(1)
    no_fast(0)


@pytest.mark.parametrize("w,D", list(FIRE_TABLE), ids=[f"u{w}x{D}" for w, D in FIRE_TABLE])
def test_derive_rows_on_the_fire_drive(sz, oracle, chunks_per_group, plan, w, D):
    """tests/fire_drive.py's batches: FIRE counters through their int16 wrap, runs replayed at frozen extreme coefficients"""
    cd, batch, data, chunk_len, nchunks = fire_batch(sz, oracle, w, D)
    with options(**OLD):
        for cpg in (1, 3):
            chunks_per_group(cpg)
            for lag in (False, True):
                fw, fu, fb = drive_forms(D, lag)
                check_case(plan, batch, "xff", w // 8, D, chunk_len, data.size, data, fw, fu, fb, (dm.I32, fm.F16)[lag], None, False, 0, cpg)
    chunks_per_group(1)


# ------------------------------------------------------------------ the filter's twin

@pytest.mark.parametrize("codec,esz,D,R", [("xff", 2, 8, 67), ("delta", 1, 5, 67), ("delta", 2, 80, 16), ("xff", 1, 16, 13)])
def test_derive_rows_is_the_twin_of_filter_linear(sz, oracle, plan, codec, esz, D, R):
    """the same form, bounds from quantiles of the model's sums: lo <= derive_rows(...) <= hi, packed as filter rows pack, is filter_linear's mask
    bit for bit and its counts, with and without a lag term"""
    rng = np.random.default_rng(D * R + esz)
    chunk_len, nchunks = D * R, 6
    n = nchunks * chunk_len - 7 * D - D // 2
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    for lag in (False, True):
        for name, w, u, bias, lo, hi in weight_sets(rng, x, esz, D, lag)[:4]:
            lo, hi = quartiles(lm.sums(x, D, w, u, bias))
            f = cd.filter_linear(batch, w.tolist(), lo=lo, hi=hi, lag_weights=None if u is None else u.tolist(), bias=int(bias))
            s = cd.derive_rows(batch, [w.tolist()], lag_forms=None if u is None else [u.tolist()], bias=int(bias)).cpu().numpy()[:, 0].astype(np.int64)
            assert np.array_equal(s, lm.sums(x, D, w, u, bias)), (name, lag)
            mask, counts = lm.pack((s >= lo) & (s <= hi), n, chunk_len, D)
            assert np.array_equal(f["mask"].cpu().numpy(), mask) and np.array_equal(f["counts"].cpu().numpy(), counts), (name, lag)
            assert 0 < counts.sum() < n // D


# ------------------------------------------------------------------ Python

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 5), ("delta", 2, 80)])
def test_derive_rows_python(sz, oracle, plan, codec, esz, D):
    """derive_rows / diff_rows against the torch expression on decompress' output, exactly; out= reuse, rets=, a side stream, the refusals"""
    import torch
    rng = np.random.default_rng(11 * D)
    chunk_len = D * 67
    n = 4 * chunk_len + 20 * D + D // 2                                            # a partial last row: no row
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    G = n // D
    flat = cd.decompress(batch).reshape(-1).view(torch.int8 if esz == 1 else torch.int16).cpu().numpy().view(DTYPES[esz])[:n]
    assert np.array_equal(flat, x)
    v = torch.from_numpy(flat[:G * D].astype(np.int32)).cuda().view(G, D)
    a, b = 0, D - 1
    # SELECT a - b, and the sum of three columns plus a bias
    family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=5, codec=CODEC_ID[codec], rows=2, out_esz=4)
    with ran(only=[family], **{family: 1}):
        got = cd.derive_rows(batch, [{a: 1, b: -1}, {0: 1, 1: 1, 2: 1}], bias=[0, 100])
    assert got.shape == (G, 2) and got.dtype == torch.int32 and got.device.type == "cuda" and got.is_contiguous()
    assert torch.equal(got, torch.stack([v[:, a] - v[:, b], v[:, 0] + v[:, 1] + v[:, 2] + 100], dim=1))
    assert torch.equal(cd.derive_rows(batch, torch.tensor([[1] + [0] * (D - 2) + [-1]]), general_layout=True)[:, 0], got[:, 0])
    # a channel minus twice its neighbour's previous value, as floats: torch's CPU expression, bit for bit
    scale, offset = dm.form_params(2)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        f = cd.derive_rows(batch, [{a: 1, b: -1}, {1: 1}], lag_forms=[0, {2: -2}], dtype=dtype, scale=scale.tolist(), offset=torch.from_numpy(offset))
        vc = v.cpu()
        s = torch.stack([vc[:, a] - vc[:, b], vc[:, 1] - 2 * torch.cat([vc[:1, 2], vc[:-1, 2]])], dim=1)
        want = (s.to(torch.float32) * torch.from_numpy(scale) + torch.from_numpy(offset)).to(dtype)
        assert f.dtype == dtype and f.shape == (G, 2)
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(f.cpu().view(bits), want.view(bits))
    # diff(): torch.diff with the first row prepended -- every column where there are at most 16, else the named ones
    cols = None if D <= 16 else [0, D // 2, D - 1]
    d = cd.diff_rows(batch, cols)
    vd = v if cols is None else v[:, cols]
    assert torch.equal(d, torch.diff(vd, dim=0, prepend=vd[:1]))
    prev = flat[:D].astype(np.int64) // 2
    d0 = cd.diff_rows(batch, cols, prev=prev.tolist())
    assert torch.equal(d0[1:], d[1:]) and d0[0].cpu().tolist() == (vd[0].cpu() - torch.from_numpy(prev if cols is None else prev[cols])).tolist()
    if D > 16:
        with pytest.raises(ValueError, match="at most 16 columns"):
            cd.diff_rows(batch)
    # out=: written in place; rets=; too small, of the wrong dtype or not contiguous is refused
    slot = batch.nchunks * 67 * 2
    out = torch.zeros(slot + 7, dtype=torch.int32, device="cuda")
    res = cd.derive_rows(batch, [{a: 1, b: -1}, {0: 1, 1: 1, 2: 1}], bias=[0, 100], out=out)
    assert res.data_ptr() == out.data_ptr() and torch.equal(res, got)
    res2 = cd.derive_rows(batch, [{a: 1}, {b: 1}], out=out)                          # the same buffer again
    assert res2.data_ptr() == out.data_ptr() and torch.equal(res2, torch.stack([v[:, a], v[:, b]], dim=1))
    rets = torch.full((batch.nchunks,), -1, dtype=torch.int64, device="cuda")
    cd.derive_rows(batch, [1], rets=rets)
    assert rets.tolist() == [min(chunk_len, n - c * chunk_len) for c in range(batch.nchunks)]
    for bad in (torch.zeros(slot - 1, dtype=torch.int32, device="cuda"), torch.zeros(slot, dtype=torch.float32, device="cuda"),
                torch.zeros(slot * 2, dtype=torch.int32, device="cuda")[::2], torch.zeros(slot, dtype=torch.int32), np.zeros(slot)):
        with pytest.raises(ValueError):
            cd.derive_rows(batch, [1, 2], out=bad)
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = cd.diff_rows(batch, cols)
    side.synchronize()
    assert torch.equal(on_side, d)
    # what Python refuses
    for kw in (dict(scale=2.0), dict(offset=1.0)):                                  # a float dtype alone takes them
        with pytest.raises(ValueError):
            cd.derive_rows(batch, [1], **kw)
    with pytest.raises(ValueError):
        cd.derive_rows(batch, [1, 2], dtype=torch.float32, scale=[1.0, 2.0, 3.0])     # K entries
    with pytest.raises(ValueError):
        cd.derive_rows(batch, [1], dtype=torch.float64)
    with pytest.raises(ValueError):
        cd.derive_rows(batch, [1] * 17)
    with pytest.raises(ValueError):
        cd.derive_rows(batch, [1], lag_forms=[1], prev=[0] * (D + 1))
    with pytest.raises(ValueError):
        sz.ChunkedCodec(codec, esz, D, chunk_len + 1, device="cuda:0").derive_rows(batch, [1])      # chunk_len % ndims != 0


def test_derive_rows_no_chunks_and_refusals(sz, gpu_lib):
    """nchunks == 0 returns 0 and launches nothing; every refusal of the header comes back with its code and names the operation, on device pointers
    as on host pointers, and launches nothing either"""
    import torch
    mem = torch.full((16384 + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    p = (mem.data_ptr() + 15) & ~15
    with ran(only=[]):
        check_refusals(gpu_lib, p)
    torch.cuda.synchronize()
    assert torch.all(mem == 0x5A)
