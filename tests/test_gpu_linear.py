"""GPU tests (-m gpu) of linear filter rows (sprintz_mi355x_filter_linear, ChunkedCodec.filter_linear / filter_change): a predicate on a
linear form over a row and its predecessor, fused into decode_fast.h and decode_kernel.h, and the seam pass behind them.  The expected
value is always tests/linear_model.py applied to the ORIGINAL input -- decode is lossless and pinned elsewhere -- and every comparison is
exact."""
import ctypes as C
import zlib

import numpy as np
import pytest

import filter_model as fm
import linear_model as lm
from dispatch import ran
from harness import DTYPES
from fixtures import no_fast, sz  # noqa: F401  (fixtures)
from rowdata import gen_data, make_batch, quartiles, weight_sets
from rowop_runners import raw_linear, run_linear

pytestmark = pytest.mark.gpu


PARITY = [
    # (esz, D, chunk_len, family)
    (1, 8, 5120, 0), (2, 8, 5120, 0),
    (1, 80, 10240, 0),                # two columns a lane
    (1, 5, 5 * 104, 0), (2, 5, 5 * 104, 0),      # lanes with columns past the last
    (2, 3, 300, 0),                   # R = 100: the last mask byte is partly padding
    (1, 4, 80, 0),                    # R = 20: the chunk is all verbatim tail
    (1, 1, 1024, 0), (2, 1, 1024, 0),
    (2, 300, 9600, 0),
    (1, 8, 5120, 1), (2, 8, 5120, 1),  # the headline shape under OPT_NO_FAST
]


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz,D,chunk_len,fam", PARITY)
def test_filter_linear_parity(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    rng = np.random.default_rng(zlib.crc32(f"{codec}{esz}{D}{chunk_len}{fam}".encode()))
    nchunks = 5
    n = nchunks * chunk_len - chunk_len // 3 - 1              # a short last chunk that ends mid-row (D = 1: mid-chunk)
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    no_fast(fam)
    nrows = n // D
    for lag in (False, True):
        for name, w, u, bias, lo, hi in weight_sets(rng, x, esz, D, lag):
            want = lm.filter_linear(x, chunk_len, D, w, lo, hi, u, bias)
            total = int(want[1].sum())
            if name in ("single", "ones", "random"):
                assert 0 < total < nrows, (name, lag, total, nrows)
            elif name == "nothing":
                assert total == 0
            mask, counts = run_linear(cd, batch, w, lo, hi, u, bias)
            msg = (codec, esz, D, chunk_len, fam, name, lag)
            assert mask.shape == want[0].shape, msg
            assert np.array_equal(counts, want[1]), ("counts",) + msg + (counts, want[1])
            assert np.array_equal(mask, want[0]), ("mask",) + msg


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [("xff", 2, 8, 5120, 0), ("delta", 1, 5, 5 * 104, 0), ("delta", 2, 8, 5120, 1)])
def test_filter_linear_wraps_as_the_header_says(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    """the C entry point with weights the Python layer refuses: the sum wraps modulo 2^32, exactly as the model's does"""
    import torch
    no_fast(fam)
    rng = np.random.default_rng(D + esz + fam)
    nchunks = 4
    n = nchunks * chunk_len - chunk_len // 3 - 1
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    MB = fm.geometry(chunk_len, D)[1]
    big = np.array([lm.INT32_MAX, lm.INT32_MIN, 0x01000000, -0x00800001, 0x7F000001, 3, -1, 0x00FFFFFF], np.int64)
    for trial in range(4):
        w = rng.permutation(big)[:D] if trial else rng.integers(lm.INT32_MIN, lm.INT32_MAX + 1, D)
        u = None if trial % 2 == 0 else rng.integers(lm.INT32_MIN, lm.INT32_MAX + 1, D)
        bias = int(rng.integers(lm.INT32_MIN, lm.INT32_MAX + 1))
        assert lm.bound_B(esz, w, u, bias) >= 1 << 31
        lo, hi = quartiles(lm.sums(x, D, w, u, bias))
        want = lm.filter_linear(x, chunk_len, D, w, lo, hi, u, bias)
        assert 0 < want[1].sum() < n // D
        dev = torch.device("cuda:0")
        w_t = torch.from_numpy(w.astype(np.int32)).to(dev)
        u_t = None if u is None else torch.from_numpy(u.astype(np.int32)).to(dev)
        tmp = torch.empty(sz._lib.filter_linear_tmp_bytes(esz, nchunks, D) // 8, dtype=torch.int64, device=dev)
        mask = torch.empty((nchunks, MB), dtype=torch.uint8, device=dev)
        counts = torch.empty(nchunks, dtype=torch.int32, device=dev)
        sz._lib.check(sz._lib.filter_linear(sz._lib.CODEC_DELTA if codec == "delta" else sz._lib.CODEC_XFF, esz, batch.data.data_ptr(),
                                            batch.offsets.data_ptr(), nchunks, chunk_len, D, w_t.data_ptr(), u_t.data_ptr() if u is not None else None,
                                            bias, lo, hi, 0, tmp.data_ptr(), mask.data_ptr(), counts.data_ptr(), None,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        assert np.array_equal(counts.cpu().numpy(), want[1]) and np.array_equal(mask.cpu().numpy(), want[0]), (codec, esz, D, fam, trial)


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [
    ("xff", 2, 8, 5120, 0), ("delta", 2, 8, 512, 0), ("delta", 1, 1, 1024, 0), ("xff", 1, 80, 10240, 0), ("delta", 2, 8, 5120, 1),
])
def test_filter_linear_seam(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    """chunk c's rows hover around a level of its own, and the levels jump by more than the threshold between chunks: a chunk's first row
    changes by more than t against its TRUE predecessor and by 0 against itself -- what the seam pass has to put right"""
    import torch
    no_fast(fam)
    rng = np.random.default_rng(D + esz)
    R = chunk_len // D
    nchunks, t, col = 12, 40, D // 2
    rows = nchunks * R - R // 3
    level = np.array([60 + 90 * (c % 2) + 3 * (c % 3) for c in range(nchunks)])              # jumps of 84 .. 96 between neighbours
    v = level[np.arange(rows) // R][:, None] + rng.integers(-3, 4, size=(rows, D))           # steps of at most 6 inside a chunk
    x = v.astype(DTYPES[esz]).ravel()
    starts = range(0, rows, R)
    up, down = lm.filter_change(x, chunk_len, D, col, lo=t + 1), lm.filter_change(x, chunk_len, D, col, hi=-t - 1)
    up0, down0 = lm.filter_change(x, chunk_len, D, col, lo=t + 1, self_rows=starts), lm.filter_change(x, chunk_len, D, col, hi=-t - 1, self_rows=starts)
    true0 = (up[0] | down[0])[1:, 0] & 1
    self0 = (up0[0] | down0[0])[1:, 0] & 1
    assert (true0 != self0).sum() * 2 >= nchunks - 1                                       # the condition, on the model
    assert not ((up[0] | down[0])[:, 1:].any()) and not (up0[0] | down0[0]).any()          # and the seams are ALL there is to find
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    g_up, g_down = cd.filter_change(batch, col, lo=t + 1), cd.filter_change(batch, col, hi=-t - 1)
    assert np.array_equal((g_up["mask"] | g_down["mask"]).cpu().numpy(), up[0] | down[0])
    assert np.array_equal(g_up["counts"].cpu().numpy(), up[1]) and np.array_equal(g_down["counts"].cpu().numpy(), down[1])
    ids = cd.filter_change(batch, col, lo=t + 1, ids=True)["ids"].cpu().numpy()
    assert np.array_equal(ids, fm.row_ids(up[0], chunk_len, D))
    # counts only (d_mask NULL: the seam pass cannot have looked at the mask) and mask only
    e = np.zeros(D, np.int64)
    e[col] = 1
    MB = fm.geometry(chunk_len, D)[1]
    for lo, hi, want in ((t + 1, None, up), (None, -t - 1, down)):
        counts = torch.full((nchunks + 8,), -77, dtype=torch.int32, device="cuda")
        raw_linear(sz, cd, batch, codec, esz, D, chunk_len, e, -e, 0, lo, hi, None, counts, None)
        k = counts.cpu().numpy()
        assert np.array_equal(k[:nchunks], want[1]) and np.all(k[nchunks:] == -77)
        mask = torch.full((nchunks * MB + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        raw_linear(sz, cd, batch, codec, esz, D, chunk_len, e, -e, 0, lo, hi, mask, None, None)
        m = mask.cpu().numpy()
        assert np.array_equal(m[:nchunks * MB].reshape(nchunks, MB), want[0]) and np.all(m[nchunks * MB:] == 0x5A)


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("fam", [0, 1])
def test_filter_linear_block_and_tail_edges(sz, oracle, no_fast, codec, esz, fam):
    """one step in one column, placed where the predecessor comes from somewhere else: the block in front, the last decoded row in front
    of the tail, the tail's previous row, and the last existing row of a short chunk.  Each is found at exactly one row."""
    no_fast(fam)
    D, R, col = 8, 64 + 5, 2                                   # four groups of 16 rows and a verbatim tail of 5
    chunk_len = D * R
    nchunks = 4
    short = 30                                                 # rows of the short last chunk: one group and a tail of 14
    rows = (nchunks - 1) * R + short
    rng = np.random.default_rng(7)
    base = 100 + rng.integers(0, 5, size=(rows, D))            # every change that is not the step is at most 4
    places = [R + 8, R + 64, R + 66, (nchunks - 1) * R + short - 1, 2 * R + 24, 2 * R + 16]
    for g in places:
        v = base.copy()
        v[g:, col] += 60                                       # the step
        v[(g // R + 1) * R:, col] -= 60                        # ... and the level is back at the next chunk, so no seam sees it
        x = np.concatenate([v.ravel(), np.full(3, 7)]).astype(DTYPES[esz])     # the batch ends mid-row
        want = lm.filter_change(x, chunk_len, D, col, lo=55)
        assert fm.row_ids(want[0], chunk_len, D).tolist() == [g], (g, fm.row_ids(want[0], chunk_len, D))     # (the way back is a change of -60)
        cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
        got = cd.filter_change(batch, col, lo=55, ids=True)
        assert got["ids"].cpu().numpy().tolist() == [g], (codec, esz, fam, g, got["ids"])
        assert np.array_equal(got["mask"].cpu().numpy(), want[0]) and np.array_equal(got["counts"].cpu().numpy(), want[1])
        down = cd.filter_change(batch, col, hi=-55, ids=True)["ids"].cpu().numpy().tolist()
        assert down == fm.row_ids(lm.filter_change(x, chunk_len, D, col, hi=-55)[0], chunk_len, D).tolist()
        assert down == ([] if g // R == nchunks - 1 else [(g // R + 1) * R])     # the way back: row 0 of the next chunk, across the seam


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("esz", [1, 2])
def test_filter_linear_long_runs(sz, oracle, no_fast, codec, esz):
    """flat spans of 3 200 rows inside a chunk (runs of 400 blocks, which the delta kernels of decode_fast.h never replay), a run from a
    chunk's first row (the zero row), a chunk that starts flat, and the step behind every run: its first row has the run's value as
    predecessor.  w + u zero (a change) and non-zero."""
    D, R = 8, 4096
    chunk_len = D * R
    top = (1 << (8 * esz)) - 1
    rng = np.random.default_rng(esz)
    nchunks = 3
    rows = nchunks * R - 700
    steps = rng.integers(-3, 4, size=(rows, D))
    v = np.mod(np.cumsum(steps, axis=0) + rng.integers(0, top, size=(1, D)), top + 1)
    flat = rng.integers(40, top - 40, D)
    for c in range(nchunks):
        v[c * R + 500:c * R + 3700] = flat
    v[R:R + 304] = 0                                           # chunk 1 starts with zero rows: a delta run from its first row
    v[2 * R:2 * R + 300] = flat                                # chunk 2 starts flat: one packed block, then a run
    v[3700] = flat + 9                                         # a step right behind chunk 0's run
    x = v.astype(DTYPES[esz]).ravel()
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    e = np.eye(D, dtype=np.int64)
    ones = np.ones(D, np.int64)
    sflat = int(flat.sum())
    sets = [("no change", e[3], -e[3], 0, 0, 0), ("change", e[3], -e[3], 0, 1, None), ("step up by 9", e[0], -e[0], 0, 9, 9),
            ("flat sum", ones, None, 0, sflat, sflat), ("flat sum, lag", ones, 2 * e[1], -2 * int(flat[1]), sflat, sflat),
            ("above flat", ones, 2 * e[1], 0, sflat + 2 * int(flat[1]) + 1, None), ("zero row", ones, ones, 5, 5, 5), ("all", ones, ones, 0, None, None)]
    for fam in (0, 1):
        no_fast(fam)
        for name, w, u, bias, lo, hi in sets:
            want = lm.filter_linear(x, chunk_len, D, w, lo, hi, u, bias)
            if name in ("no change", "flat sum", "flat sum, lag"):
                assert want[1][0] >= 3199, (name, want[1])
            if name == "zero row":
                assert want[1][1] >= 303
            if name == "step up by 9":
                assert fm.row_ids(want[0], chunk_len, D)[0] == 3700
            mask, counts = run_linear(cd, batch, w, lo, hi, u, bias)
            assert np.array_equal(counts, want[1]), (codec, esz, fam, name, counts, want[1])
            assert np.array_equal(mask, want[0]), (codec, esz, fam, name)


@pytest.mark.parametrize("codec,esz,D,chunk_len", [("xff", 2, 8, 5120), ("delta", 1, 80, 10240), ("delta", 1, 1, 1024), ("xff", 2, 5, 520), ("delta", 2, 300, 9600)])
def test_filter_linear_equals_filter_rows_on_one_column(sz, oracle, codec, esz, D, chunk_len):
    """weights = e_d and no lag: the box filter on column d alone, byte for byte"""
    rng = np.random.default_rng(D)
    n = 6 * chunk_len - chunk_len // 2 - (1 if D > 1 else 0)
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    top = (1 << (8 * esz)) - 1
    for d in sorted({0, D // 2, D - 1}):
        col = x[:n // D * D].reshape(-1, D)[:, d].astype(np.int64)
        for lo, hi in (quartiles(col), (int(col.min()), int(col.min())), (0, top), (top, 0)):
            lo_v, hi_v = [None] * D, [None] * D
            lo_v[d], hi_v[d] = lo, hi
            box = cd.filter_rows(batch, lo_v, hi_v, mode="all")
            lin = cd.filter_linear(batch, {d: 1}, lo=lo, hi=hi)
            assert box["mask"].equal(lin["mask"]) and box["counts"].equal(lin["counts"]), (codec, esz, D, d, lo, hi)


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam,family", [
    ("xff", 2, 8, 5120, 0, "dec_fast"),
    ("delta", 2, 8, 5120, 0, "dec_fast"),
    ("delta", 1, 1, 1024, 0, "dec_generic"),      # decode_uni is not taught the mode
    ("xff", 2, 2, 1024, 0, "dec_generic"),
    ("delta", 2, 300, 9600, 0, "dec_generic"),
    ("xff", 2, 8, 5120, 1, "dec_generic"),
])
def test_filter_linear_which_kernel(sz, oracle, no_fast, codec, esz, D, chunk_len, fam, family):
    no_fast(fam)
    rng = np.random.default_rng(D + fam)
    n = 6 * chunk_len - 7 * D - (3 if D > 1 else 0)
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    for lag in (False, True):
        name, w, u, bias, lo, hi = weight_sets(rng, x, esz, D, lag)[0]
        with ran(only=[family], **{family: 1}):               # one decode launch; the seam pass is no kernel family
            mask, counts = run_linear(cd, batch, w, lo, hi, u, bias, check=False)
        want = lm.filter_linear(x, chunk_len, D, w, lo, hi, u, bias)
        assert np.array_equal(mask, want[0]) and np.array_equal(counts, want[1])


GUARD_SHAPES = [
    # test_gpu_filter.py's, less the shape only decode_uni ragged rows have; whole rows a chunk, as the operation asks
    ("xff", 2, 8, 5120),          # decode_fast
    ("delta", 1, 1, 1024),        # decode_kernel, one column
    ("delta", 2, 300, 9600),      # decode_kernel
]


@pytest.mark.parametrize("codec,esz,D,chunk_len", GUARD_SHAPES)
def test_filter_linear_output_guards(sz, oracle, codec, esz, D, chunk_len):
    """sentinel-filled, padded outputs and scratch: nothing lands past nchunks*MB / nchunks / tmp_bytes, every byte inside mask and counts
    is written, either output may be NULL"""
    import torch
    from sprintz_amd import _lib
    rng = np.random.default_rng(D)
    nchunks = 7
    n = nchunks * chunk_len - chunk_len // 2 - (1 if D > 1 else 0)
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    MB = fm.geometry(chunk_len, D)[1]
    pad = 4096
    tb = _lib.filter_linear_tmp_bytes(esz, nchunks, D)
    for lag in (False, True):
        for name, w, u, bias, lo, hi in weight_sets(rng, x, esz, D, lag)[:3]:
            want = lm.filter_linear(x, chunk_len, D, w, lo, hi, u, bias)
            for sent in (0x5A, 0xA5):                          # two sentinels: a byte that equals one of them by value was still written
                for outs in ("both", "mask", "counts"):
                    mask = torch.full((nchunks * MB + pad,), sent, dtype=torch.uint8, device="cuda")
                    counts = torch.full((nchunks + 64,), -77, dtype=torch.int32, device="cuda")
                    rets = torch.full((nchunks + 1,), -77, dtype=torch.int64, device="cuda")
                    tmp = torch.full((tb + pad,), sent, dtype=torch.uint8, device="cuda")
                    raw_linear(sz, cd, batch, codec, esz, D, chunk_len, w, u, bias, lo, hi, mask if outs != "counts" else None,
                               counts if outs != "mask" else None, rets, tmp)
                    r = rets.cpu().numpy()
                    assert np.array_equal(r[:nchunks], [min(chunk_len, n - c * chunk_len) for c in range(nchunks)]) and r[nchunks] == -77
                    m, k, s = mask.cpu().numpy(), counts.cpu().numpy(), tmp.cpu().numpy()
                    assert np.all(m[nchunks * MB:] == sent) and np.all(k[nchunks:] == -77) and np.all(s[tb:] == sent), (codec, D, name, outs, "padding")
                    if not lag:
                        assert np.all(s == sent), "scratch written without a lag term"
                    if outs != "counts":
                        assert np.array_equal(m[:nchunks * MB].reshape(nchunks, MB), want[0]), (codec, D, name, lag, outs, sent)
                    else:
                        assert np.all(m == sent), "a NULL mask was written"
                    if outs != "mask":
                        assert np.array_equal(k[:nchunks], want[1]), (codec, D, name, lag, outs)
                    else:
                        assert np.all(k == -77), "NULL counts were written"


@pytest.mark.parametrize("codec,esz,D,chunk_len,fam", [
    ("xff", 2, 8, 5120, 0),       # decode_fast
    ("delta", 1, 1, 1024, 0),     # decode_kernel, one column
    ("delta", 1, 80, 10240, 0),   # decode_fast, 2 columns a lane
    ("xff", 2, 8, 5120, 1),       # decode_kernel (NO_FAST)
])
def test_filter_linear_damaged_chunk(sz, oracle, no_fast, codec, esz, D, chunk_len, fam):
    """rets names the damaged chunk and check=True raises; the chunks in front are right.  Nothing is said about row 0 of the chunk behind
    it (its predecessor is gone); the rest of that chunk and every later chunk are right too."""
    import torch
    no_fast(fam)
    rng = np.random.default_rng(5)
    nchunks = 9
    n = nchunks * chunk_len - 100
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    bad = 4
    off = int(batch.offsets[bad].item())
    hdr = batch.data[off + 6:off + 8].clone()
    batch.data[off + 6] = hdr[0] ^ 0x5                  # the header's ndims field
    MB = fm.geometry(chunk_len, D)[1]
    for lag in (False, True):
        name, w, u, bias, lo, hi = weight_sets(rng, x, esz, D, lag)[0]
        want = lm.filter_linear(x, chunk_len, D, w, lo, hi, u, bias)
        mask = torch.full((nchunks * MB + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        counts = torch.full((nchunks + 8,), -77, dtype=torch.int32, device="cuda")
        rets = torch.empty(nchunks, dtype=torch.int64, device="cuda")
        raw_linear(sz, cd, batch, codec, esz, D, chunk_len, w, u, bias, lo, hi, mask, counts, rets)
        r = rets.cpu().numpy()
        assert r[bad] < 0
        assert all(r[c] == min(chunk_len, n - c * chunk_len) for c in range(nchunks) if c != bad)
        m, k = mask.cpu().numpy(), counts.cpu().numpy()
        assert np.all(m[nchunks * MB:] == 0x5A) and np.all(k[nchunks:] == -77)        # nothing outside the outputs
        m = m[:nchunks * MB].reshape(nchunks, MB)
        assert np.array_equal(m[:bad], want[0][:bad]) and np.array_equal(k[:bad], want[1][:bad])
        assert np.array_equal(m[bad + 2:], want[0][bad + 2:]) and np.array_equal(k[bad + 2:nchunks], want[1][bad + 2:])
        behind = m[bad + 1].copy()
        behind[0] = (behind[0] & 0xFE) | (want[0][bad + 1, 0] & 1)                      # (row 0 behind the damage: unspecified)
        assert np.array_equal(behind, want[0][bad + 1])
        ul = None if u is None else [int(e) for e in u]
        with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):
            cd.filter_linear(batch, [int(e) for e in w], lo=lo, hi=hi, lag_weights=ul, bias=bias, check=True)
        cd.filter_linear(batch, [int(e) for e in w], lo=lo, hi=hi, lag_weights=ul, bias=bias, check=False)      # no error without the check
        with pytest.raises(sz.SprintzError, match=f"chunk {bad} "):                   # ... but ids are sized and placed by the counts: they check
            cd.filter_linear(batch, [int(e) for e in w], lo=lo, hi=hi, lag_weights=ul, bias=bias, ids=True, check=False)
    batch.data[off + 6] = hdr[0]
    mask, counts = run_linear(cd, batch, w, lo, hi, u, bias)                           # repaired: no error, and exact
    assert np.array_equal(mask, want[0]) and np.array_equal(counts, want[1])


@pytest.mark.parametrize("codec,esz,D,chunk_len", [("xff", 2, 8, 5120), ("delta", 1, 16, 2048), ("delta", 2, 3, 300)])
def test_filter_linear_feeds_select_rows(sz, oracle, codec, esz, D, chunk_len):
    """the mask is the common currency: select_rows on a filter_linear mask -- alone, and AND-ed with a filter_rows mask -- returns exactly
    the model's rows and their numbers"""
    rng = np.random.default_rng(D * 3 + esz)
    n = 5 * chunk_len - chunk_len // 3 - 1
    x = gen_data("walk", rng, n, esz, D)
    cd, batch = make_batch(sz, oracle, codec, esz, D, chunk_len, x, False)
    v = x[:n // D * D].reshape(-1, D)
    top = (1 << (8 * esz)) - 1
    f = cd.filter_linear(batch, {0: 1, D - 1: -1}, lo=1)                               # WHERE a > b
    want_ids = np.flatnonzero(v[:, 0].astype(np.int64) > v[:, D - 1].astype(np.int64))
    got = cd.select_rows(batch, f["mask"], counts=f["counts"], ids=True)
    assert np.array_equal(got["ids"].cpu().numpy(), want_ids)
    assert np.array_equal(got["rows"].cpu().numpy().view(DTYPES[esz]), v[want_ids])
    c = cd.filter_change(batch, 1, lo=1)                                               # ... AND column 1 went up AND column 0 in its upper half
    lo_v = [None] * D
    lo_v[0] = top // 2
    b = cd.filter_rows(batch, lo_v, None)
    d1 = np.diff(v[:, 1].astype(np.int64), prepend=int(v[0, 1]))
    want_ids = np.flatnonzero((v[:, 0].astype(np.int64) > v[:, D - 1].astype(np.int64)) & (d1 >= 1) & (v[:, 0] >= top // 2))
    got = cd.select_rows(batch, f["mask"] & c["mask"] & b["mask"], ids=True)
    assert np.array_equal(got["ids"].cpu().numpy(), want_ids)
    assert np.array_equal(got["rows"].cpu().numpy().view(DTYPES[esz]), v[want_ids])
