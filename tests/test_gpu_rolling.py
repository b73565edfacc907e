"""GPU tests (-m gpu) of rolling rows (sprintz_mi355x_rolling_rows, ChunkedCodec.rolling_rows): per element, its column's min / max / sum
over the W rows that end at its row, straight from a compressed batch.

The expected value is always the numpy model (tests/rolling_model.py) on the ORIGINAL input, compared exactly.  Every launch runs on
sentinel-filled outputs, scratch and rets with padding around them, and asserts its kernel family (tests/dispatch.py) against the
planner's answer for the shape (tests/plan_probe.cpp, asked with q=15 rows=W out_esz=...)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import planner
import rolling_model as rm
from drive_tables import ROWOP_CASES, ROWOP_IDS, fire_batch, rowop_batch
from drive_tables import FIRE_SHAPES as FIRE_TABLE
from fixtures import chunks_per_group, no_fast, sz  # noqa: F401  (fixtures)
from rowdata import FLOAT_FAST_SHAPES as FAST_SHAPES, GENERIC_SHAPES, gen_data, lowdim, make_batch
from streams import OLD, options, truncated_batch
from dispatch import ran
from harness import DTYPES

pytestmark = pytest.mark.gpu

PAD = 1024                                             # sentinel elements in front of and behind every output
TPAD = 256                                             # sentinel bytes in front of and behind the seam scratch
SENT = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A}
CODEC_ID = {"delta": 0, "xff": 1}
Q_ROLLING = 15
WINDOWS = (8, 16, 64)


@pytest.fixture(scope="module")
def plan():
    """the planner on a host compiler: -> f(**fields) -> the family's name"""
    planner.available(required=True)

    def ask(**fields):
        got = planner.ask("decode", q=Q_ROLLING, **fields)
        assert got.get("family") in ("dec_fast", "dec_generic"), got
        return got["family"]
    return ask


def out_esz(esz, ops):
    return 4 if ops & rm.SUM else esz


def run_rolling(batch, codec, esz, D, chunk_len, W, ops, general=False, shift=0):
    """the C entry point on sentinel-filled buffers: each selected output has PAD + shift elements in front, nchunks * chunk_len of its own
    and PAD behind; the scratch TPAD bytes around it; rets one entry behind.  -> ({op: the whole buffer}, rets [nchunks + 1])"""
    import torch
    from sprintz_amd import _lib
    n = batch.nchunks
    bufs, ptrs = {}, {}
    for name in ("min", "max", "sum"):
        if not ops & rm.OPS[name]:
            ptrs[name] = None
            continue
        osz = 4 if name == "sum" else esz
        dt = {1: torch.int8, 2: torch.int16, 4: torch.int32}[osz]
        bufs[name] = torch.full((PAD + shift + n * chunk_len + PAD,), SENT[osz], dtype=dt, device="cuda")
        ptrs[name] = bufs[name].data_ptr() + (PAD + shift) * osz
    tbytes = n * rm.tmp_stride(W, D, esz) if n > 1 else 0
    tmp = torch.full((TPAD + tbytes + TPAD,), 0xA5, dtype=torch.uint8, device="cuda")
    rets = torch.full((n + 1,), -77, dtype=torch.int64, device="cuda")
    _lib.check(_lib.rolling_rows(CODEC_ID[codec], esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, chunk_len, D, W, ops,
                                 _lib.QUERY_GENERAL_LAYOUT if general else 0, ptrs["min"], ptrs["max"], ptrs["sum"],
                                 tmp.data_ptr() + TPAD if n > 1 else None, rets.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    t = tmp.cpu().numpy()
    assert np.all(t[:TPAD] == 0xA5) and np.all(t[TPAD + tbytes:] == 0xA5), "written around the seam scratch"
    udt = {1: np.uint8, 2: np.uint16, 4: np.int32}
    return {k: v.cpu().numpy().view(udt[v.element_size()]) for k, v in bufs.items()}, rets.cpu().numpy()


def assert_rolling(h, rets, x, chunk_len, nchunks, D, W, want, ops, shift, msg, bad=(), local=None):
    """every selected output against the model's `want`: the chunks outside `bad` are the model's -- the first W - 1 rows of a chunk behind a
    bad one are `local`'s, the chunk-local model's -- nothing is written in front, behind, or past the short last chunk's count; rets are
    the chunks' element counts (outside `bad`), with the sentinel behind"""
    n, ne = x.size, nchunks * chunk_len
    assert set(h) == set(rm.names(ops)), (sorted(h),) + msg
    e = np.arange(n)
    keep = np.ones(n, bool)
    behind = np.zeros(n, bool)
    for c in bad:
        keep[c * chunk_len:(c + 1) * chunk_len] = False
        behind |= (e // chunk_len == c + 1) & (e % chunk_len // D < W - 1)
    for name, buf in h.items():
        sent = SENT[buf.dtype.itemsize]
        assert buf.size == PAD + shift + ne + PAD
        assert np.all(buf[:PAD + shift] == sent), (name, "written in front") + msg
        assert np.all(buf[PAD + shift + ne:] == sent), (name, "written behind") + msg
        body = buf[PAD + shift:PAD + shift + ne]
        assert np.all(body[n:] == sent), (name, "written past the last chunk's count") + msg
        exact = keep & ~behind
        ne_ = body[:n][exact] != want[name][exact]
        assert not ne_.any(), (name, int(ne_.sum()), "of", int(exact.sum()), "elements differ; first at", int(np.flatnonzero(exact)[np.flatnonzero(ne_)[0]])) + msg
        if behind.any():
            assert np.array_equal(body[:n][behind & keep], local[name][behind & keep]), (name, "the chunk behind a damaged one is not chunk-local") + msg
    lens = [min(chunk_len, n - c * chunk_len) for c in range(nchunks)]
    assert all(rets[c] == lens[c] for c in range(nchunks) if c not in bad) and all(rets[c] < 0 for c in bad) and rets[nchunks] == -77, ("rets", rets.tolist()) + msg


def rotate(key, k):
    return zlib.crc32(key.encode()) % k


def named_chunk_len(D):
    """67 rows: four groups of 16 and a verbatim tail of 3 rows; W = 64 leaves 3 rows of a chunk with a full window inside it"""
    return D * (16 * 4 + 3)


# ------------------------------------------------------------------ parity

@pytest.mark.parametrize("codec,esz,D", [(codec, esz, D) for codec in ("delta", "xff") for esz, D in FAST_SHAPES + GENERIC_SHAPES])
def test_rolling_rows_parity_named_shapes(sz, oracle, no_fast, chunks_per_group, plan, codec, esz, D):
    """the sixteen shapes named for the planner, both codecs, both families (NO_FAST), 1 and 3 chunks a lane group -- decode_fast.h's chunk loop,
    where the ring restarts cold with every chunk -- with and without the general layout, W = 8 / 16 / 64, every subset of the ops; a short
    last chunk of 5 rows (fewer than W - 1) or one that ends mid-row.  67 rows: four groups, so that decode_fast.h takes the shapes it serves"""
    key = f"roll{codec}{esz}{D}"
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    chunk_len = named_chunk_len(D)
    nchunks = 5 + D % 4
    last = 5 * D if rotate(key, 2) or D == 1 else 37 * D + max(1, D // 2)
    n = (nchunks - 1) * chunk_len + last
    x = gen_data(("walk", "uniform", "sparse")[rotate(key, 3)], rng, n, esz, D)
    batches = {False: make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)[1]}
    batches[True] = make_batch(sz, oracle, codec, esz, D, chunk_len, x, True)[1] if lowdim(esz, D) else batches[False]
    seen = set()
    for W in WINDOWS:
        want = rm.rolling(x, D, W)
        for general in (False, True):
            for fam in (0, 1):
                no_fast(fam)
                for cpg in (1, 3):
                    chunks_per_group(cpg)
                    for ops in (rm.SUBSETS if (fam, cpg) == (0, 1) else (7,)):
                        family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], rows=W, out_esz=out_esz(esz, ops),
                                      general=general, no_fast=fam, chunks_per_group=cpg)
                        assert family == ("dec_fast" if rm.fast_takes(esz, D, chunk_len, W, general, fam, 0, out_esz(esz, ops)) else "dec_generic")
                        seen.add(family)
                        with ran(only=[family], **{family: 1}):
                            h, rets = run_rolling(batches[general], codec, esz, D, chunk_len, W, ops, general)
                        assert_rolling(h, rets, x, chunk_len, nchunks, D, W, want, ops, 0, (codec, esz, D, W, general, fam, cpg, ops, family))
    assert ("dec_fast" in seen) == ((esz, D) in ((2, 8), (2, 16), (2, 24), (2, 64), (1, 16))) and "dec_generic" in seen
    chunks_per_group(1)


# ------------------------------------------------------------------ data chosen to break the step

def ramp(esz, D, G, falling):
    """a strictly falling (rising) ramp down every column, another phase a column, wrapping in the element type: the minimum (maximum) is
    the newest row and the maximum (minimum) the row about to leave -- the oldest block's suffix and the newest block's prefix at every j"""
    r = np.arange(G, dtype=np.int64)[:, None] + 3 * np.arange(D, dtype=np.int64)[None, :]
    return np.mod((1 << (8 * esz)) - 1 - r if falling else r, 1 << (8 * esz)).astype(DTYPES[esz]).reshape(-1)


@pytest.mark.parametrize("codec,esz,D", [("delta", 2, 8), ("xff", 2, 8), ("xff", 1, 16), ("delta", 1, 3), ("xff", 2, 5)])
@pytest.mark.parametrize("falling", [True, False], ids=["falling", "rising"])
def test_rolling_rows_on_ramps(sz, oracle, plan, codec, esz, D, falling):
    chunk_len = named_chunk_len(D)
    nchunks = 5
    x = ramp(esz, D, nchunks * 67 - 20, falling)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    for W in WINDOWS:
        want = rm.rolling(x, D, W)
        if esz == 2:                                      # (no wrap inside 16 bits: the ramp's own rule, checked on the model)
            g, d = np.arange(x.size) // D, np.arange(x.size) % D
            oldest = x[np.maximum(g - W + 1, 0) * D + d]
            assert np.array_equal(want["min" if falling else "max"], x) and np.array_equal(want["max" if falling else "min"], oldest)
        family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], rows=W, out_esz=4)
        with ran(only=[family], **{family: 1}):
            h, rets = run_rolling(batch, codec, esz, D, chunk_len, W, 7)
        assert_rolling(h, rets, x, chunk_len, nchunks, D, W, want, 7, 0, (codec, esz, D, W, falling))


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("D,general", [(8, False), (1, False), (1, True)])
def test_rolling_rows_all_ones_at_the_largest_window(sz, oracle, plan, codec, D, general):
    """uint16 columns of all 65535 at the largest W the shape takes: the sum's top bits, delta runs far longer than the window"""
    esz = 2
    W = rm.max_window(esz, D, general)
    R = W + 11
    chunk_len, nchunks = D * R, 4
    x = np.full(nchunks * chunk_len - 3 * D, 65535, np.uint16)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, general)
    want = rm.rolling(x, D, W)
    assert int(want["sum"].max()) == W * 65535 > 1 << 24
    family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], rows=W, out_esz=4, general=general)
    with ran(only=[family], **{family: 1}):
        h, rets = run_rolling(batch, codec, esz, D, chunk_len, W, 7, general)
    assert_rolling(h, rets, x, chunk_len, nchunks, D, W, want, 7, 0, (codec, D, W, general))
    # one window more is refused, and the refusal names the largest
    with pytest.raises(sz.SprintzError, match=f"largest window_rows allowed is {W}$"):
        sz.ChunkedCodec(codec, esz, D, D * (W + 16), device="cuda:0").rolling_rows(batch, W + 8, general_layout=general)


@pytest.mark.parametrize("codec,w,D,kind", ROWOP_CASES, ids=ROWOP_IDS)
def test_rolling_rows_over_runs(sz, oracle, chunks_per_group, plan, codec, w, D, kind):
    """tests/rle_drive.py's batches: runs of 1 .. 16 blocks and maximal ones -- shorter than the window, longer, beginning mid-window, at
    chunk starts and ending at the chunk's last block; on the planner's family for the shape (decode_fast.h at 1 and 3 chunks a lane group for
    u16 x 8 and u8 x 32) and on the generic kernel"""
    cd, batch, data, chunk_len, _ = rowop_batch(sz, oracle, codec, w, D, kind)
    with options(**OLD):
        for W in (8, 64):
            want = rm.rolling(data, D, W)
            for cpg in (1, 3):
                chunks_per_group(cpg)
                family = plan(esz=w // 8, D=D, chunk_len=chunk_len, nchunks=batch.nchunks, codec=CODEC_ID[codec], rows=W, out_esz=4, chunks_per_group=cpg)
                with ran(only=[family], **{family: 1}):
                    h, rets = run_rolling(batch, codec, w // 8, D, chunk_len, W, 7)
                assert_rolling(h, rets, data, chunk_len, batch.nchunks, D, W, want, 7, 0, (codec, w, D, kind, W, cpg))
    chunks_per_group(1)


@pytest.mark.parametrize("esz,D", [(2, 8), (1, 3), (2, 1)])
def test_rolling_rows_delta_run_settles(sz, oracle, plan, esz, D):
    """the run shortcut's edges under the delta codec: a chunk that starts inside a run, runs of exactly W + 8 rows and one block more or
    less (the ring is full of one value from the W + 8-th row of a run on), a run that begins mid-window behind moving rows and ends at the
    chunk's last block, and a step between two runs"""
    rng = np.random.default_rng(esz * 100 + D)
    R, nchunks = 16 * 14, 4
    chunk_len = D * R
    for W in (8, 64):
        rows = np.zeros((nchunks, R, D), np.int64)
        rows[0, :] = 7 + np.arange(D)                                              # one run, the whole chunk
        for c, extra in ((1, 0), (2, 8), (3, -8)):
            moving = R - (W + 8 + extra) - 24
            rows[c, :moving] = rng.integers(0, 200, (moving, D))
            rows[c, moving:] = 50 + c + np.arange(D)                               # a run of W + 8 + extra + 24 rows to the chunk's end ...
            rows[c, moving + W + 8 + extra:] += 3                                  # ... with a step W + 8 + extra rows into it
        x = rows.reshape(-1).astype(DTYPES[esz])
        cd, batch = make_batch(sz, oracle, "delta", esz, D, chunk_len, x, False)
        family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=0, rows=W, out_esz=4)
        for ops in (7, 2):
            with ran(only=[family], **{family: 1}):
                h, rets = run_rolling(batch, "delta", esz, D, chunk_len, W, ops)
            assert_rolling(h, rets, x, chunk_len, nchunks, D, W, rm.rolling(x, D, W), ops, 0, (esz, D, W, ops))


@pytest.mark.parametrize("w,D", list(FIRE_TABLE), ids=[f"u{w}x{D}" for w, D in FIRE_TABLE])
def test_rolling_rows_on_the_fire_drive(sz, oracle, plan, w, D):
    """tests/fire_drive.py's batches: FIRE counters through their int16 wrap, runs replayed at frozen extreme coefficients"""
    cd, batch, data, chunk_len, nchunks = fire_batch(sz, oracle, w, D)
    with options(**OLD):
        for W, ops in ((16, 7), (64, 5)):
            family = plan(esz=w // 8, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=1, rows=W, out_esz=4)
            with ran(only=[family], **{family: 1}):
                h, rets = run_rolling(batch, "xff", w // 8, D, chunk_len, W, ops)
            assert_rolling(h, rets, data, chunk_len, nchunks, D, W, rm.rolling(data, D, W), ops, 0, ("fire", w, D, W))


# ------------------------------------------------------------------ seams

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 16), ("delta", 2, 3), ("xff", 1, 1)])
def test_rolling_rows_over_the_chunk_seams(sz, oracle, plan, codec, esz, D):
    """every chunk's rows differ from its neighbour's -- high chunks and low chunks in turn -- so that the chunk-local result differs from
    the true one in each of the first W - 1 rows: the sum everywhere, the minimum behind a low chunk, the maximum behind a high one.  Then
    one chunk alone, where no seam pass runs and no scratch is needed, and chunk 0's clipped windows against the definition"""
    rng = np.random.default_rng(D)
    chunk_len, nchunks = named_chunk_len(D), 6
    n = nchunks * chunk_len - 9 * D
    level = np.where(np.arange(n) // chunk_len % 2 == 0, 100, 10)
    x = (level + rng.integers(1, 21, n)).astype(DTYPES[esz])
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    e = np.arange(n)
    for W in WINDOWS:
        want, local = rm.rolling(x, D, W), rm.rolling_local(x, chunk_len, D, W)
        seam = (e >= chunk_len) & (e % chunk_len // D < W - 1)
        high = e // chunk_len % 2 == 0
        assert np.all(want["sum"][seam] != local["sum"][seam])
        assert np.all(want["min"][seam & high] != local["min"][seam & high]) and np.all(want["max"][seam & ~high] != local["max"][seam & ~high])
        family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], rows=W, out_esz=4)
        with ran(only=[family], **{family: 1}):
            h, rets = run_rolling(batch, codec, esz, D, chunk_len, W, 7)
        assert_rolling(h, rets, x, chunk_len, nchunks, D, W, want, 7, 0, (codec, esz, D, W))
        # chunk 0's clipped windows, against the definition itself
        first = rm.brute(x[:W * D], D, W)
        for k in ("min", "max", "sum"):
            assert np.array_equal(h[k][PAD:PAD + W * D], first[k]), (k, W)
    one = x[:chunk_len - 2 * D - D // 2]
    cd1, b1 = make_batch(sz, oracle, codec, esz, D, chunk_len, one, False)
    assert b1.nchunks == 1
    for W in WINDOWS:
        family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=1, codec=CODEC_ID[codec], rows=W, out_esz=4)
        with ran(only=[family], **{family: 1}):
            h, rets = run_rolling(b1, codec, esz, D, chunk_len, W, 7)
        assert_rolling(h, rets, one, chunk_len, 1, D, W, rm.rolling(one, D, W), 7, 0, (codec, esz, D, W, "one chunk"))


# ------------------------------------------------------------------ the edges of the buffers

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 16), ("delta", 2, 5), ("xff", 1, 7)])
def test_rolling_rows_edges_of_the_buffers(sz, oracle, plan, codec, esz, D):
    """outputs off the 16-byte grid by one element and by 16, a last chunk that ends mid-row: nothing is written outside the outputs (run_rolling
    checks the scratch's padding at every launch), nor past the last chunk's count, and d_rets keeps the sentinel behind it"""
    rng = np.random.default_rng(7 * D)
    chunk_len, nchunks = D * (16 * 5 + 11), 6
    n = (nchunks - 1) * chunk_len + D * 37 + max(1, D // 2)
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    for W in (8, 64):
        want = rm.rolling(x, D, W)
        for shift in (0, 1, 16):
            for ops in (7, 1, 4):
                family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], rows=W, out_esz=out_esz(esz, ops), out_lo=(shift * esz) % 16)
                with ran(only=[family], **{family: 1}):
                    h, rets = run_rolling(batch, codec, esz, D, chunk_len, W, ops, False, shift)
                assert_rolling(h, rets, x, chunk_len, nchunks, D, W, want, ops, shift, (codec, esz, D, W, shift, ops))


# ------------------------------------------------------------------ damage

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 32), ("delta", 2, 12)])
def test_rolling_rows_damaged_chunk(sz, oracle, chunks_per_group, plan, codec, esz, D):
    """one truncated chunk in the middle: its rets entry is negative and every other chunk's is its count (decompress_batch's); the chunks
    not adjacent to it are exact, the chunk behind it is exact from row W - 1 on and chunk-local in front; check=True names the chunk"""
    import torch
    rng = np.random.default_rng(3 * D)
    chunk_len, nchunks, cut = named_chunk_len(D), 7, 3
    n = nchunks * chunk_len - 5 * D
    x = gen_data("walk", rng, n, esz, D)
    cd, good = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    batch = truncated_batch(sz, good, cut)
    with options(**OLD):
        chunks_per_group(3)
        plain_rets = torch.full((nchunks,), -77, dtype=torch.int64, device="cuda")
        cd.decompress(batch, rets=plain_rets)
        plain_rets = plain_rets.cpu().numpy()
        assert plain_rets[cut] < 0 and np.all(np.delete(plain_rets, cut) > 0)
        for W in WINDOWS:
            family = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, codec=CODEC_ID[codec], rows=W, out_esz=4, chunks_per_group=3)
            with ran(only=[family], **{family: 1}):
                h, rets = run_rolling(batch, codec, esz, D, chunk_len, W, 7)
            assert np.array_equal(rets[:nchunks], plain_rets), (rets.tolist(), plain_rets.tolist())
            assert_rolling(h, rets, x, chunk_len, nchunks, D, W, rm.rolling(x, D, W), 7, 0, (codec, esz, D, W), bad=(cut,), local=rm.rolling_local(x, chunk_len, D, W))
        with pytest.raises(sz.SprintzError, match=f"rolling_rows: chunk {cut} "):
            cd.rolling_rows(batch, 16)
        got = cd.rolling_rows(batch, 16, check=False)
        assert got["sum"].shape == (n // D, D)
        cd.rolling_rows(good, 16)                                                  # undamaged: no error
    chunks_per_group(1)


# ------------------------------------------------------------------ refusals

def test_rolling_rows_refusals(sz, oracle):
    import torch
    from sprintz_amd import _lib
    esz, D, R = 2, 8, 400
    chunk_len = D * R
    x = gen_data("walk", np.random.default_rng(2), 3 * chunk_len, esz, D)
    cd, batch = make_batch(sz, oracle, "xff", esz, D, chunk_len, x, False)
    for W in (0, 4, 12, 63, R + 8, 408):                                           # not a multiple of 8; above R
        with pytest.raises(ValueError):
            cd.rolling_rows(batch, W)
    wmax = rm.max_window(esz, D, False)
    assert wmax + 8 <= R
    with pytest.raises(sz.SprintzError, match=f"largest window_rows allowed is {wmax}$") as info:      # over the LDS bound
        cd.rolling_rows(batch, wmax + 8)
    assert info.value.code == _lib.E_UNSUPPORTED
    for ops in ((), ("median",), ("min", "range")):
        with pytest.raises(ValueError):
            cd.rolling_rows(batch, 8, ops=ops)
    with pytest.raises(ValueError):
        sz.ChunkedCodec("xff", 2, 8, chunk_len + 3, device="cuda:0").rolling_rows(batch, 8)      # chunk_len % ndims != 0
    # the C entry point: a mismatched ops / pointer pair, misaligned outputs -- nothing launches, nothing is written
    n = batch.nchunks
    out = torch.full((n * chunk_len + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    tmp = torch.empty(n * rm.tmp_stride(8, D, esz), dtype=torch.uint8, device="cuda")
    p = out.data_ptr()

    def call(ops, mn, mx, sm, t=tmp.data_ptr()):
        return _lib.rolling_rows(1, esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, chunk_len, D, 8, ops, 0, mn, mx, sm, t, None,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    with ran(only=[]):
        assert call(7, p, p, None) == _lib.E_INVALID and call(3, p, None, None) == _lib.E_INVALID      # an op without its output
        assert call(1, p, None, p) == _lib.E_INVALID and call(4, p, None, p) == _lib.E_INVALID         # an output without its op
        assert call(1, p + 1, None, None) == _lib.E_INVALID and call(2, None, p + 3, None) == _lib.E_INVALID and call(4, None, None, p + 2) == _lib.E_INVALID
        assert call(4, None, None, p, None) == _lib.E_INVALID and call(4, None, None, p, tmp.data_ptr() + 8) == _lib.E_INVALID      # the scratch
        assert "rolling_rows" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.all(out == 0x5A5A5A5A)


# ------------------------------------------------------------------ Python

@pytest.mark.parametrize("codec,esz,D", [("xff", 2, 8), ("delta", 1, 5)])
def test_rolling_rows_python(sz, oracle, codec, esz, D):
    import torch
    rng = np.random.default_rng(11 * D)
    chunk_len = named_chunk_len(D)
    n = 5 * chunk_len + 20 * D + D // 2                                            # a partial last row
    x = gen_data("uniform", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    G = -(-n // D)

    def flat(t):
        return t.cpu().numpy().reshape(-1)
    for W in (8, 64):
        want = rm.rolling(x, D, W)
        family = "dec_fast" if rm.fast_takes(esz, D, chunk_len, W) else "dec_generic"
        with ran(only=[family], **{family: 1}):                                    # one library call: the decode launch and its seam pass
            got = cd.rolling_rows(batch, W, ops=("min", "max", "sum", "mean"))
        assert list(got) == ["min", "max", "sum", "mean"] and all(v.shape == (G, D) and v.device.type == "cuda" for v in got.values())
        assert got["min"].dtype == got["max"].dtype == cd.dtype and got["sum"].dtype == torch.int32 and got["mean"].dtype == torch.float32
        view = torch.int8 if esz == 1 else torch.int16
        for k in ("min", "max"):
            assert np.array_equal(flat(got[k].view(view)).view(DTYPES[esz])[:n], want[k]) and not flat(got[k].view(view))[n:].any()
        assert np.array_equal(flat(got["sum"])[:n], want["sum"]) and not flat(got["sum"])[n:].any()
        assert np.array_equal(flat(got["mean"])[:n].view(np.uint32), rm.mean(want["sum"], D, W).view(np.uint32))
        # defaults; one op by name; the mean alone comes from the sum launch
        assert list(cd.rolling_rows(batch, W)) == ["min", "max", "sum"]
        only = cd.rolling_rows(batch, W, ops="mean", general_layout=True)
        assert list(only) == ["mean"] and torch.equal(only["mean"], got["mean"])
        assert torch.equal(cd.rolling_rows(batch, W, ops=("max",))["max"].view(view), got["max"].view(view))
