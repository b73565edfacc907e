"""CPU tests of aggregate rows (sprintz_mi355x_aggregate_rows): the symbol and its binding are there, every validation return comes
before the device is touched and names the operation, the numpy model the GPU tier compares with (tests/aggregate_model.py) equals a
one-row-at-a-time brute force, the windowed query's model under an all-ones mask and the filter model's counts, and the planner
(sprintz_amd/csrc/plan.h, built with g++: tests/plan_probe.cpp) sends the mode where the windowed query
goes -- except that decode_uni.h never gets it."""
import os

import numpy as np
import pytest

import aggregate_model as am
import filter_model as fm
import window_model as wm
from fixtures import buf_fixture, lib, random_mask, refusals  # noqa: F401  (fixtures)
from planner import QUERY, family, plan_fixture

HERE = os.path.dirname(os.path.abspath(__file__))
Q_WINDOW, Q_AGGREGATE = QUERY["window"], QUERY["aggregate"]


buf = buf_fixture(16384)


def test_symbol_and_binding(lib):
    assert "sprintz_mi355x_aggregate_rows" in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.lib, "sprintz_mi355x_aggregate_rows")
    assert len(lib.aggregate_rows.argtypes) == 17
    assert (lib.AGG_MIN, lib.AGG_MAX, lib.AGG_SUM, lib.AGG_COUNT) == (1, 2, 4, 8)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_aggregate_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    for name, v in (("MIN", 1), ("MAX", 2), ("SUM", 4), ("COUNT", 8)):
        assert f"#define SPRINTZ_AGG_{name} {v}u" in hdr
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    from sprintz_amd import ChunkedCodec
    assert callable(ChunkedCodec.aggregate_rows) and callable(ChunkedCodec.aggregate_where)


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=5120, D=8, mask=p + 128, W=64, ops=15, flags=0, mn=p + 2048, mx=p + 4096,
                sm=p + 6144, cnt=p + 8192, rets=p + 10240)

    def call(**kw):
        a = dict(good, **kw)
        return lib.aggregate_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["mask"], a["W"], a["ops"],
                                  a["flags"], a["mn"], a["mx"], a["sm"], a["cnt"], a["rets"], None)

    invalid, unsupported = refusals(lib, call, "aggregate_rows")

    invalid(cl=5121)                                                             # chunk_len % ndims != 0
    invalid(D=7)
    invalid(cl=0)                                                                # chunk_len outside 1..2^30
    invalid(cl=(1 << 30) + 8)
    for W in (0, 4, 7, 12, 63, 65):                                              # W not a multiple of 8 that is >= 8
        invalid(W=W)
    for ops in (0, 16, 17, 32, 0xFFFFFFFF):                                      # ops outside 1..15
        invalid(ops=ops)
    for k, bit in (("mn", 1), ("mx", 2), ("sm", 4), ("cnt", 8)):                 # a selected output that is NULL
        invalid(**{k: None})
        invalid(**{k: None, "ops": bit})
    for k in ("comp", "offs", "mask"):                                           # NULL pointers
        invalid(**{k: None})
    invalid(mn=p + 2049)                                                         # d_min / d_max not aligned to the element size
    invalid(mx=p + 4097)
    for off in (1, 2, 3):
        invalid(cnt=p + 8192 + off)                                              # d_count not aligned to 4 bytes
    for off in (1, 2, 4):
        invalid(sm=p + 6144 + off)                                               # d_sum / d_rets not aligned to 8 bytes
        invalid(rets=p + 10240 + off)
    invalid(flags=2)                                                             # unknown flag (GENERAL_LAYOUT = 1 is the only one)
    invalid(flags=3)
    assert call(D=0) == E.E_INVALID and call(codec=9) == E.E_INVALID and call(esz=3) == E.E_INVALID
    unsupported(D=513, cl=513 * 16)                                              # more than 512 columns
    for codec in (2, 3):
        unsupported(codec=codec)                                                 # the non-RLE codecs
    unsupported(codec=4, esz=1)
    assert call(n=0) == 0                                                        # nothing to do: returns 0, launches nothing
    import torch
    if not torch.cuda.is_available():
        assert call() == E.E_NO_DEVICE
        for k, bit in (("mn", 1), ("mx", 2), ("sm", 4), ("cnt", 8)):             # an output that is not selected may be NULL
            assert call(**{k: None, "ops": 15 & ~bit}) == E.E_NO_DEVICE, k
        assert call(mn=None, mx=None, sm=None, ops=8) == E.E_NO_DEVICE           # the count alone
        assert call(mn=p + 2049, ops=14) == E.E_NO_DEVICE                        # ... and may lie anywhere
        assert call(rets=None) == E.E_NO_DEVICE
        assert call(esz=1, mn=p + 2049, mx=p + 4097, mask=p + 129) == E.E_NO_DEVICE   # 8-bit outputs and the mask may lie anywhere
        assert call(W=648) == E.E_NO_DEVICE and call(W=1 << 20) == E.E_NO_DEVICE # W > R: one aggregate a chunk
        assert call(flags=1, D=512, cl=512 * 16) == E.E_NO_DEVICE


SHAPES = [
    # (esz, D, chunk_len, n): whole rows and short last chunks (one ending mid-row), R % 8 != 0 and R < 8
    (1, 3, 3 * 33, 3 * 33 * 4 + 3 * 14),
    (2, 5, 5 * 21, 5 * 21 * 3 + 5 * 4 + 2),
    (1, 1, 13, 13 * 5 + 6),
    (2, 8, 8 * 64, 8 * 64 * 3),
    (1, 7, 7 * 5, 7 * 5 * 6 + 7),
]


def windows_for(R):
    r8 = -(-R // 8) * 8
    return sorted({8, 24, r8, r8 + 8})


def assert_same(got, want, msg):
    for k in ("min", "max", "sum", "count"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k].astype(np.uint64), want[k].astype(np.uint64)), (k,) + msg


@pytest.mark.parametrize("esz,D,chunk_len,n", SHAPES)
def test_model_equals_brute_force(esz, D, chunk_len, n):
    rng = np.random.default_rng(n + D)
    x = rng.integers(0, 1 << (8 * esz), n).astype(np.uint8 if esz == 1 else np.uint16)
    R, MB = fm.geometry(chunk_len, D)
    nchunks = -(-n // chunk_len)
    for p in (0.0, 0.03, 0.5, 1.0):
        mask = random_mask(rng, nchunks, MB, p)              # bits of rows that do not exist are set too: they are ignored
        for W in windows_for(R):
            got = am.aggregate_rows(x, chunk_len, D, mask, W)
            assert_same(got, am.aggregate_rows_brute(x, chunk_len, D, mask, W), (p, W))
            assert got["min"].dtype == x.dtype and got["sum"].dtype == np.uint64 and got["count"].dtype == np.uint32
            assert got["count"].shape == (nchunks, -(-R // W))
            empty = got["count"] == 0
            assert np.all(got["min"][empty] == (1 << (8 * esz)) - 1) and np.all(got["max"][empty] == 0) and np.all(got["sum"][empty] == 0)
            if p == 0.0:
                assert empty.all()


@pytest.mark.parametrize("esz,D,chunk_len,n", [s for s in SHAPES if s[3] % s[1] == 0])
def test_model_with_every_bit_set_is_the_windowed_query(esz, D, chunk_len, n):
    rng = np.random.default_rng(n)
    x = rng.integers(0, 1 << (8 * esz), n).astype(np.uint8 if esz == 1 else np.uint16)
    R, MB = fm.geometry(chunk_len, D)
    nchunks = -(-n // chunk_len)
    ones = np.full((nchunks, MB), 0xFF, np.uint8)
    for W in windows_for(R):
        got = am.aggregate_rows(x, chunk_len, D, ones, W)
        mn, mx, sm = wm.chunk_windows(x, chunk_len, D, W)
        assert np.array_equal(got["min"], mn) and np.array_equal(got["max"], mx) and np.array_equal(got["sum"], sm), W
        assert int(got["count"].sum()) == n // D


@pytest.mark.parametrize("esz,D,chunk_len,n", SHAPES)
def test_model_counts_are_the_filter_models(esz, D, chunk_len, n):
    rng = np.random.default_rng(n + 1)
    top = (1 << (8 * esz)) - 1
    x = rng.integers(0, top + 1, n).astype(np.uint8 if esz == 1 else np.uint16)
    R, MB = fm.geometry(chunk_len, D)
    lo, hi = np.zeros(D, np.int64), np.full(D, top, np.int64)
    lo[0], hi[D - 1] = top // 4, 3 * top // 4
    for mode in (fm.ALL, fm.ANY):
        mask, cnt = fm.filter_rows(x, chunk_len, D, lo if mode == fm.ALL else hi, hi if mode == fm.ALL else lo + top // 2, mode)
        for W in windows_for(R):
            got = am.aggregate_rows(x, chunk_len, D, mask, W)
            assert np.array_equal(got["count"].sum(axis=1), cnt), (mode, W)
            bits = np.unpackbits(mask, axis=1, bitorder="little")[:, :R]
            nwin = -(-R // W)
            per_window = np.pad(bits, ((0, 0), (0, nwin * W - R))).reshape(-1, nwin, W).sum(axis=2)
            assert np.array_equal(got["count"], per_window), (mode, W)


def test_global_model_folds_the_chunk_windows():
    rng = np.random.default_rng(3)
    D, R = 4, 24
    chunk_len = D * R
    n = chunk_len * 5 + D * 7
    x = rng.integers(0, 256, n).astype(np.uint8)
    mask = random_mask(rng, 6, 3, 0.3)
    for W in (8, 24, 48, 72):                                # R % W == 0 and W % R == 0
        g = am.global_windows(x, chunk_len, D, mask, W)
        sel = am.selected(mask, n, chunk_len, D).reshape(-1)
        rows = np.pad(x, (0, 6 * chunk_len - n)).reshape(-1, D)
        for w in range(g["count"].size):
            pick = np.flatnonzero(sel[w * W:(w + 1) * W]) + w * W
            assert g["count"][w] == pick.size
            assert np.array_equal(g["sum"][w], rows[pick].sum(axis=0))
            if pick.size:
                assert np.array_equal(g["min"][w], rows[pick].min(axis=0)) and np.array_equal(g["max"][w], rows[pick].max(axis=0))
                assert np.allclose(g["mean"][w], rows[pick].mean(axis=0))
            else:
                assert np.all(g["min"][w] == 255) and np.all(g["max"][w] == 0) and np.all(np.isnan(g["mean"][w]))


plan = plan_fixture(shape=family, codec=1, nchunks=4096, q=Q_AGGREGATE)


def test_planner_edges(plan):
    # where the windowed query goes to decode_fast.h, so does the mode: reduce only, so no condition on the output or on whole 16-byte rows
    fast = [(1, 16, 16 * 512), (2, 8, 5120), (1, 80, 10240), (2, 24, 24 * 200), (1, 8, 4096), (2, 4, 4096), (1, 24, 24 * 200),
            (2, 128, 128 * 80), (1, 256, 256 * 80), (2, 5, 5 * 1024), (2, 3, 3000)]
    for esz, D, cl in fast:
        for codec in (0, 1):
            assert plan(esz=esz, D=D, chunk_len=cl, codec=codec, q=Q_WINDOW) == "dec_fast", (esz, D, cl)
            assert plan(esz=esz, D=D, chunk_len=cl, codec=codec) == "dec_fast", (esz, D, cl)
        assert plan(esz=esz, D=D, chunk_len=cl, no_fast=1) == "dec_generic", (esz, D, cl)
        for out_lo in (1, 2, 8, 15):                       # (there is no output to align)
            assert plan(esz=esz, D=D, chunk_len=cl, out_lo=out_lo) == "dec_fast", (esz, D, cl, out_lo)
    # the low-dimension layouts: decode_uni.h serves the windowed query and is not taught this mode
    for esz, D, cl in [(1, 1, 1024), (2, 1, 1024), (1, 2, 2048), (2, 2, 2048), (1, 3, 3000), (1, 4, 4096)]:
        assert plan(esz=esz, D=D, chunk_len=cl, q=Q_WINDOW) == "dec_uni", (esz, D, cl)
        assert plan(esz=esz, D=D, chunk_len=cl) == "dec_generic", (esz, D, cl)
        assert plan(esz=esz, D=D, chunk_len=cl, no_fast=1) == "dec_generic", (esz, D, cl)
    # everything else the windowed query leaves to the generic kernel: more than 256 columns, group less than half full, blocks that
    # are not whole 16-byte pieces, chunks shorter than the read-ahead ring
    for esz, D, cl in [(2, 300, 9600), (1, 300, 9600), (1, 512, 512 * 16), (2, 33, 33 * 64), (1, 5, 5 * 1024), (1, 33, 33 * 128), (2, 8, 8 * 13)]:
        for general in (0, 1):
            want = plan(esz=esz, D=D, chunk_len=cl, general=general, q=Q_WINDOW)
            assert want == "dec_generic", (esz, D, cl, general)
            assert plan(esz=esz, D=D, chunk_len=cl, general=general) == want, (esz, D, cl, general)
    # general layout asked for on a low-dimension shape: the windowed query's rule decides
    for esz, D, cl in [(1, 4, 4096), (2, 2, 2048), (1, 1, 1024)]:
        assert plan(esz=esz, D=D, chunk_len=cl, general=1) == plan(esz=esz, D=D, chunk_len=cl, general=1, q=Q_WINDOW)
    # the mode never reaches the small-batch, block-parallel or univariate kernels, whatever the batch size
    for nchunks in (1, 64, 2048, 2049, 131072):
        assert plan(esz=2, D=8, chunk_len=5120, nchunks=nchunks) == "dec_fast"
        assert plan(esz=1, D=80, chunk_len=10240, nchunks=nchunks, codec=0) == "dec_fast"
        assert plan(esz=1, D=1, chunk_len=1024, nchunks=nchunks, codec=0) == "dec_generic"
    # the other modes' plans are what they were
    assert plan(esz=1, D=1, chunk_len=1024, q=5) == "dec_uni" and plan(esz=1, D=1, chunk_len=1024, q=6) == "dec_generic"
    assert plan(esz=2, D=8, chunk_len=5120, q=6, capacity=10) == "dec_fast"
