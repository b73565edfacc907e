"""CPU tier of FIR rows (sprintz_mi355x_fir_rows, ChunkedCodec.fir_rows): the symbols and their bindings are there, every validation return
comes before the device is touched, the numpy model the GPU tier compares with (tests/fir_model.py) agrees with numpy.convolve per column, with
derive rows' diff at T = 2 and with rolling rows' sum for taps of ones, rowops.fir_taps follows it, and the planner (sprintz_amd/csrc/plan.h,
built with g++: tests/plan_probe.cpp, asked with q=19 rows=T out_esz=...) sends the mode to decode_fast.h while rings and taps fit its LDS
budget and to the generic kernel otherwise -- both sides of every edge, computed here from geom.h's formulas restated in Python."""
import os

import numpy as np
import pytest

import derive_model as dm
import fir_model as fm
import planner
import rolling_model as rm
from fir_runner import check_refusals
from fixtures import buf_fixture, lib  # noqa: F401  (fixtures)
from rowdata import FLOAT_FAST_SHAPES as FAST_SHAPES, GENERIC_SHAPES, RAGGED_SHAPES

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = {1: np.uint8, 2: np.uint16}
Q_FIR = 19                                                # geom.h: kQueryFir
TAPS = [1, 2, 3, 9, 10, 17, 65, 68]


buf = buf_fixture(16384)


def test_symbols_and_bindings(lib):
    for name in ("sprintz_mi355x_fir_rows_tmp_bytes", "sprintz_mi355x_fir_rows"):
        assert name in lib.EXPORTED_SYMBOLS and hasattr(lib.lib, name)
    assert len(lib.fir_rows.argtypes) == 19 and len(lib.fir_rows_tmp_bytes.argtypes) == 4
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "uint64_t sprintz_mi355x_fir_rows_tmp_bytes(int elem_bytes, uint64_t nchunks, uint16_t ndims, uint32_t ntaps);" in hdr
    assert "int sprintz_mi355x_fir_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    assert "uint32_t chunk_len, uint16_t ndims, uint32_t ntaps," in hdr
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    geom = open(os.path.join(os.path.dirname(HERE), "sprintz_amd", "csrc", "geom.h")).read()
    assert f"kQueryFir = {Q_FIR};" in geom
    from sprintz_amd import ChunkedCodec
    for name in ("fir_rows", "shift_rows", "lag_diff_rows", "smooth_rows"):
        assert callable(getattr(ChunkedCodec, name))


def test_validation_comes_before_the_device(lib, buf):
    check_refusals(lib, buf[1])


def test_tmp_bytes(lib):
    from sprintz_amd import rowops
    for esz, n, D, T in ((2, 5, 8, 9), (1, 7, 3, 2), (2, 1, 8, 65), (1, 3, 80, 256), (2, 0, 8, 9)):
        assert lib.fir_rows_tmp_bytes(esz, n, D, T) == n * fm.tmp_stride(T, D, esz) == rowops.fir_tmp_bytes(n, T, D, esz)
        assert fm.tmp_stride(T, D, esz) % 16 == 0 and fm.tmp_stride(T, D, esz) >= 16 + 2 * (T - 1) * D * esz
    assert lib.fir_rows_tmp_bytes(2, 5, 8, 1) == 0 == rowops.fir_tmp_bytes(5, 1, 8, 2)      # one tap: no scratch


# ------------------------------------------------------------------ the model

@pytest.mark.parametrize("esz,D,chunk_len,n", RAGGED_SHAPES)
def test_model_is_numpy_convolve_per_column(esz, D, chunk_len, n):
    """int64 convolution of every column with its own taps: with prev, with a prev of zeros (scipy.signal.lfilter's initial state) and with the
    edge replicated; and the brute-force loop"""
    rng = np.random.default_rng(n + D)
    x = rng.integers(0, 1 << (8 * esz), n).astype(DTYPES[esz])
    G = n // D
    xr = x[:G * D].reshape(G, D).astype(np.int64)
    for T in (1, 2, 3, 9, 17):
        t, b = fm.random_taps(rng, T, D, esz)
        prevs = [("prev", rng.integers(0, 1 << (8 * esz), (T - 1, D)).astype(DTYPES[esz])), ("zeros", np.zeros((T - 1, D), DTYPES[esz])), ("edge", None)]
        for name, prev in prevs:
            got = fm.sums(x, D, t, b, prev)
            front = np.repeat(xr[:1], T - 1, axis=0) if prev is None else prev.astype(np.int64)
            for d in range(D):
                col = np.concatenate([front[:, d], xr[:, d]])
                want = np.convolve(col, t[:, d])[T - 1:T - 1 + G] + b[d]
                assert np.array_equal(got[:G * D].reshape(G, D)[:, d], want), (name, T, d)
            assert np.array_equal(got, fm.sums_brute(x, D, t, b, prev)), (name, T)
    # shared taps broadcast
    assert np.array_equal(fm.sums(x, D, [1, -2, 1]), fm.sums(x, D, np.repeat(np.array([[1], [-2], [1]]), D, axis=1)))


@pytest.mark.parametrize("esz,D,chunk_len,n", RAGGED_SHAPES)
def test_model_meets_derive_and_rolling(esz, D, chunk_len, n):
    """T = 2 with taps e_d and -e_d is derive_model's diff; taps of W ones with a prev of zeros is rolling_model's sum; the wrap is modulo 2^32"""
    rng = np.random.default_rng(3 * n + D)
    x = rng.integers(0, 1 << (8 * esz), n).astype(DTYPES[esz])
    G = n // D
    e = np.eye(D, dtype=np.int64)
    for prev in (None, rng.integers(0, 1 << (8 * esz), D).astype(DTYPES[esz])):
        want = dm.sums(x, D, e, -e, None, prev)
        got = fm.sums(x, D, [1, -1], None, None if prev is None else prev.reshape(1, D))
        assert np.array_equal(got[:G * D].reshape(G, D), want)
    for W in (8, 16, 24):
        got = fm.sums(x, D, np.ones(W, np.int64), None, np.zeros((W - 1, D), DTYPES[esz]))
        assert np.array_equal(got, rm.rolling(x, D, W)["sum"].astype(np.int64))
    t, b = fm.random_taps(rng, 5, D, esz, exact=False)
    assert max(fm.bound(esz, t, b, D)) >= 1 << 31
    assert np.array_equal(fm.sums(x, D, t, b), fm.sums_brute(x, D, t, b))
    # the chunk-local variant differs from the batch's only in the first T - 1 rows of a chunk
    t, b = fm.random_taps(rng, 4, D, esz)
    loc, glob = fm.sums_local(x, chunk_len, D, t, b), fm.sums(x, D, t, b)
    rows = np.arange(n) % chunk_len // D
    assert np.array_equal(loc[rows >= 3], glob[rows >= 3])


def test_model_float_formats_follow_derive_rows():
    rng = np.random.default_rng(5)
    D, n = 5, 5 * 40 + 3
    x = rng.integers(0, 65536, n).astype(np.uint16)
    t, b = fm.random_taps(rng, 3, D, 2)
    scale, offset = dm.form_params(D)
    y = fm.sums(x, D, t, b)
    assert np.abs(y).max() > 1 << 24                                           # sums the float32 conversion rounds
    for fmt in fm.FORMATS:
        bits = fm.fir_rows(x, D, t, b, fmt, scale, offset)
        assert bits.shape == (n,) and bits.dtype == dm.BITS_DTYPE[fmt]
        whole = dm.convert(y[:n // D * D].reshape(-1, D), fmt, scale, offset).reshape(-1)
        assert np.array_equal(bits[:whole.size], whole)


# ------------------------------------------------------------------ rowops

def test_fir_taps_and_wrappers():
    import torch
    from sprintz_amd import rowops
    t, b = rowops.fir_taps([1, 2, 1], 0, 4, 2, "cpu")
    assert t.dtype == torch.int32 and t.shape == (3, 4) and t.is_contiguous() and t.tolist() == [[1] * 4, [2] * 4, [1] * 4] and b.tolist() == [0] * 4
    t, b = rowops.fir_taps([[1, 2], [3, 4]], [5, -6], 2, 1, "cpu")
    assert t.tolist() == [[1, 2], [3, 4]] and b.tolist() == [5, -6]
    t, _ = rowops.fir_taps(torch.tensor([[1, 2], [3, 4]], dtype=torch.int64), 0, 2, 1, "cpu")
    assert t.tolist() == [[1, 2], [3, 4]]
    t, _ = rowops.fir_taps(torch.tensor([7, -7]), 0, 3, 1, "cpu")
    assert t.tolist() == [[7] * 3, [-7] * 3]
    # the bound at its edge, on both sides: |bias| + (2^W - 1) sum |taps| < 2^31
    for esz in (1, 2):
        top = (1 << (8 * esz)) - 1
        q = ((1 << 31) - 1) // top
        left = (1 << 31) - 1 - q * top
        rowops.fir_taps([q - 5, -5], [left, -left], 2, esz, "cpu")             # B = 2^31 - 1 in both columns
        assert fm.bound(esz, [q - 5, -5], [left, -left], 2) == [(1 << 31) - 1] * 2
        with pytest.raises(ValueError, match="column 1's filter can reach 2147483648 in magnitude"):
            rowops.fir_taps([q - 5, -5], [left, -left - 1], 2, esz, "cpu")
        with pytest.raises(ValueError, match="must stay below 2\\^31"):
            rowops.fir_taps([[q, 0], [1, 0]], 0, 2, esz, "cpu")
    for bad in ([], [1] * 257, 3, {0: 1}, [[1, 2, 3]], [1.5, 2], torch.tensor([1.0]), torch.zeros((2, 3), dtype=torch.int32), None):
        with pytest.raises(ValueError):
            rowops.fir_taps(bad, 0, 2, 1, "cpu")
    with pytest.raises(ValueError):
        rowops.fir_taps([1], [0, 0, 0], 2, 1, "cpu")
    assert rowops.shift_taps(0) == [1] and rowops.shift_taps(3) == [0, 0, 0, 1]
    assert rowops.lag_diff_taps(1) == [1, -1] and rowops.lag_diff_taps(4) == [1, 0, 0, 0, -1]
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            rowops.shift_taps(bad)
    for bad in (0, 256):
        with pytest.raises(ValueError):
            rowops.lag_diff_taps(bad)
    # the wrappers' taps through the model: shift and lag difference
    x = np.arange(40, dtype=np.uint16) * 3 % 17
    assert np.array_equal(fm.sums(x, 2, rowops.shift_taps(3))[6:], x[:-6]) and np.array_equal(fm.sums(x, 2, rowops.shift_taps(3))[:6], np.tile(x[:2], 3))
    assert np.array_equal(fm.sums(x, 2, rowops.lag_diff_taps(2))[4:], x[4:].astype(np.int64) - x[:-4])


# ------------------------------------------------------------------ the planner

@pytest.fixture(scope="module")
def plan():
    planner.available()
    return lambda **fields: planner.ask("decode", q=Q_FIR, **fields)


def named_chunk_len(D):
    return D * (16 * 4 + 3)


@pytest.mark.parametrize("esz,D", FAST_SHAPES + GENERIC_SHAPES)
def test_planner_family_and_lds(plan, esz, D):
    """the family for every named shape, from the planner's rules restated in fir_model: decode_fast.h for rows of whole 16-byte pieces on a
    one-column-a-lane mapping (8 .. 64 columns) with the chunk's ring behind the groups' carves at table_off and the taps behind the rings, the
    generic kernel -- the rings alone as its LDS -- for everything else and under NO_FAST; misaligned outputs go to the generic kernel"""
    chunk_len = named_chunk_len(D)
    seen = set()
    for general in (0, 1):
        dp = rm.lanes(esz, D, general)
        fdp, _, carve = rm.fast_map(esz, D)
        for T in TAPS:
            for out_esz in (4, 2):
                for no_fast in (0, 1):
                    for cpg in (1, 3):
                        for out_lo in (0, 4):
                            got = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=7, codec=1, rows=T, out_esz=out_esz, general=general, no_fast=no_fast,
                                       chunks_per_group=cpg, out_lo=out_lo)
                            ring = fm.ring_bytes(T, D, esz)
                            if fm.fast_takes(esz, D, chunk_len, T, general, no_fast, out_lo, out_esz):
                                groups = rm.THREADS // fdp
                                assert got.get("family") == "dec_fast", got
                                assert got["lds_group_stride"] == carve and got["table_off"] == carve * groups, got
                                assert got["lds"] == (carve + ring) * groups + 4 * T * D == fm.fast_lds(esz, D, T), got
                                assert got["dp"] == fdp and got["cpl"] == 1 and got["chunks_per_group"] == cpg and got["grid"] == -(--(-7 // cpg) * fdp // rm.THREADS), got
                            else:
                                assert got.get("family") == "dec_generic", got
                                assert got["lds_group_stride"] == ring and got["lds"] == ring * (rm.THREADS // dp) and got["table_off"] == 0, got
                                assert got["log2DP"] == dp.bit_length() - 1 and got["grid"] == -(-7 * dp // rm.THREADS) and got["vec_store"] == 0, got
                            seen.add(got["family"])
    assert seen == ({"dec_fast", "dec_generic"} if (esz, D) in ((2, 8), (2, 16), (2, 24), (2, 64), (1, 16)) else {"dec_generic"})


@pytest.mark.parametrize("esz,D", [(2, 8), (2, 16), (2, 24), (2, 32), (1, 16), (1, 32), (1, 64)])
def test_planner_hands_over_at_the_fast_lds_budget(plan, esz, D):
    """both sides of the edge (f.ring + ring) x groups + 4 T D <= kHistFastLdsBudget, from the geometry functions: the largest such T runs
    decode_fast.h, the next one the generic kernel"""
    dp, cpl, carve = rm.fast_map(esz, D)
    t = fm.fast_max_taps(esz, D)
    assert cpl == 1 and 1 <= t
    assert fm.fast_lds(esz, D, t) <= rm.FAST_LDS_BUDGET
    chunk_len = D * 320
    inside = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=5, codec=0, rows=t, out_esz=4)
    assert inside.get("family") == "dec_fast" and inside["lds"] == fm.fast_lds(esz, D, t) and inside["table_off"] == carve * (rm.THREADS // dp), inside
    if t < fm.MAX_TAPS:
        assert fm.fast_lds(esz, D, t + 1) > rm.FAST_LDS_BUDGET and t + 1 <= fm.max_taps(esz, D, False)
        beyond = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=5, codec=0, rows=t + 1, out_esz=4)
        assert beyond.get("family") == "dec_generic" and beyond["lds"] == fm.ring_bytes(t + 1, D, esz) * (rm.THREADS // rm.lanes(esz, D, False)), beyond
    if (esz, D) == (2, 8):                                                       # the headline shape: 65 taps are inside
        assert t >= 65


@pytest.mark.parametrize("esz,D", FAST_SHAPES + GENERIC_SHAPES + [(2, 512), (1, 300)])
def test_planner_refusals(plan, esz, D):
    """T - 1 > R, T outside 1 .. 256, a non-RLE codec; and both sides of the edge where the rings of a workgroup's chunks stop fitting its 160 KB"""
    for general in (0, 1):
        tmax = fm.max_taps(esz, D, general)
        groups = rm.THREADS // rm.lanes(esz, D, general)
        assert 1 <= tmax <= fm.MAX_TAPS
        assert fm.ring_bytes(tmax, D, esz) * groups <= rm.LDS_MAX
        chunk_len = D * 320
        inside = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=3, codec=0, rows=tmax, out_esz=4, general=general, no_fast=1)
        assert inside.get("family") == "dec_generic" and inside["lds"] == fm.ring_bytes(tmax, D, esz) * groups, inside
        if tmax < fm.MAX_TAPS:
            assert fm.ring_bytes(tmax + 1, D, esz) * groups > rm.LDS_MAX
            beyond = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=3, codec=0, rows=tmax + 1, out_esz=4, general=general)
            assert beyond.get("error") == -4 and "fir_rows" in beyond["what"], beyond              # SPRINTZ_E_UNSUPPORTED
    for bad in (0, 257, 1000):
        got = plan(esz=esz, D=D, chunk_len=D * 2000, nchunks=3, codec=0, rows=bad, out_esz=4)
        assert got.get("error") == -1 and "fir_rows" in got["what"], got
    got = plan(esz=esz, D=D, chunk_len=D * 16, nchunks=3, codec=0, rows=18, out_esz=4)               # T - 1 = 17 > R = 16
    assert got.get("error") == -1 and "fir_rows" in got["what"], got
    assert "family" in plan(esz=esz, D=D, chunk_len=D * 16, nchunks=3, codec=0, rows=17, out_esz=4, no_fast=1)      # T - 1 = R
    for codec in (2, 3):
        got = plan(esz=esz, D=D, chunk_len=D * 64, nchunks=3, codec=codec, rows=3, out_esz=4)
        assert got.get("error") == -4 and "fir_rows" in got["what"], got


def test_planner_refuses_more_than_512_columns(plan):
    got = plan(esz=1, D=513, chunk_len=513 * 64, nchunks=3, codec=0, rows=3, out_esz=4)
    assert got.get("error") == -4 and "fir_rows" in got["what"], got


def test_planner_leaves_the_other_modes_alone():
    base = dict(esz=2, D=8, chunk_len=5120, nchunks=4096, codec=1)
    assert planner.ask("decode", **base) == planner.ask("decode", rows=65, **base)
    # rolling rows, whose ring and budget the mode shares, keeps its plan: the fast kernel with its own LDS, no table of taps behind the rings
    dp, _, carve = rm.fast_map(2, 8)
    roll = planner.ask("decode", q=15, rows=64, out_esz=4, **base)
    assert roll.get("family") == "dec_fast" and roll["lds"] == (carve + rm.ring_bytes(64, 8, 2)) * (rm.THREADS // dp) and roll["table_off"] == carve * (rm.THREADS // dp), roll
