"""CPU tests of histogram rows (sprintz_mi355x_histogram_rows): the symbol and its binding are there, every validation return comes
before the device is touched and names the operation, the numpy model the GPU tier compares with (tests/histogram_model.py) equals
np.bincount / np.sort brute force, and the planner (sprintz_amd/csrc/plan.h, built with g++: tests/plan_probe.cpp) sends the
mode to decode_fast.h where the windowed query goes AND the table fits the launch's LDS next to the groups' carves, to the generic
kernel otherwise -- never to decode_uni.h."""
import os

import numpy as np
import pytest

import filter_model as fm
import histogram_model as hm
import planner
from fixtures import buf_fixture, lib, random_mask, refusals  # noqa: F401  (fixtures)
from planner import QUERY

HERE = os.path.dirname(os.path.abspath(__file__))
Q_WINDOW, Q_AGGREGATE, Q_HISTOGRAM = QUERY["window"], QUERY["aggregate"], QUERY["histogram"]
CAP = 16384
FAST_LDS_BUDGET = 80 * 1024           # geom.h: kHistFastLdsBudget


buf = buf_fixture(16384)


def test_symbol_and_binding(lib):
    assert "sprintz_mi355x_histogram_rows" in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.lib, "sprintz_mi355x_histogram_rows")
    assert len(lib.histogram_rows.argtypes) == 16
    assert lib.HIST_MAX_COUNTERS == CAP
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_histogram_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    assert "#define SPRINTZ_HIST_MAX_COUNTERS 16384u" in hdr
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    from sprintz_amd import ChunkedCodec
    assert callable(ChunkedCodec.histogram_rows) and callable(ChunkedCodec.histogram_where) and callable(ChunkedCodec.quantiles)


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=5120, D=8, mask=p + 128, lo=p + 512, shift=8, nbins=256, H=0, flags=0,
                hist=p + 2048, rets=p + 10240)

    def call(**kw):
        a = dict(good, **kw)
        return lib.histogram_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["mask"], a["lo"], a["shift"],
                                  a["nbins"], a["H"], a["flags"], a["hist"], a["rets"], None)

    invalid, unsupported = refusals(lib, call, "histogram_rows")

    invalid(cl=5121)                                                             # chunk_len % ndims != 0
    invalid(D=7)
    invalid(cl=0)                                                                # chunk_len outside 1..2^30
    invalid(cl=(1 << 30) + 8)
    for shift in (16, 17, 32, 0xFFFFFFFF):                                       # 0 <= shift < W
        invalid(shift=shift)
    for shift in (8, 9, 31):
        invalid(esz=1, shift=shift, nbins=1)
    invalid(nbins=0)                                                             # 1 <= nbins <= 2^(W - shift)
    invalid(nbins=257)                                                           # (shift 8 at 16 bits: 256 bins are the range)
    invalid(shift=15, nbins=3)
    invalid(esz=1, shift=0, nbins=257)
    invalid(esz=1, shift=4, nbins=17)
    invalid(hist=None)                                                           # NULL pointers
    for k in ("comp", "offs"):
        invalid(**{k: None})
    for off in (1, 2, 4):                                                        # d_hist / d_rets not aligned to 8 bytes
        invalid(hist=p + 2048 + off)
        invalid(rets=p + 10240 + off)
    invalid(lo=p + 513)                                                          # d_lo not aligned to the element size
    invalid(n=(1 << 29) + 1, H=1)                                                # more than 2^40 entries of d_hist: 2^29 + 1 histograms of 8 x 256
    invalid(n=1 << 40, H=1)
    invalid(n=(1 << 40) + 1, H=2, D=512, cl=512 * 16, nbins=32, shift=11)
    invalid(flags=2)                                                             # unknown flag (GENERAL_LAYOUT = 1 is the only one)
    invalid(flags=3)
    assert call(D=0) == E.E_INVALID and call(codec=9) == E.E_INVALID and call(esz=3) == E.E_INVALID
    # the cap, both sides of 16384 counters
    unsupported(D=8, shift=0, nbins=2049)
    unsupported(D=65, cl=65 * 16, shift=8, nbins=256)
    unsupported(esz=1, D=80, cl=80 * 16, shift=0, nbins=256)
    unsupported(D=512, cl=512 * 16, shift=8, nbins=33)
    unsupported(D=513, cl=513 * 16, nbins=1)                                     # more than 512 columns
    for codec in (2, 3):
        unsupported(codec=codec)                                                 # the non-RLE codecs
    unsupported(codec=4, esz=1, shift=0)
    assert call(n=0) == 0                                                        # nothing to do: returns 0, launches nothing
    assert call(n=0, mask=None, lo=None, rets=None) == 0
    import torch
    if not torch.cuda.is_available():
        assert call() == E.E_NO_DEVICE
        assert call(D=8, shift=0, nbins=2048) == E.E_NO_DEVICE                   # exactly the cap
        assert call(D=64, cl=64 * 16, shift=8, nbins=256) == E.E_NO_DEVICE
        assert call(esz=1, D=80, cl=80 * 16, shift=0, nbins=128, lo=p + 513) == E.E_NO_DEVICE      # (8-bit lo may lie anywhere)
        assert call(D=512, cl=512 * 16, shift=8, nbins=32, flags=1) == E.E_NO_DEVICE
        assert call(mask=None) == E.E_NO_DEVICE and call(lo=None) == E.E_NO_DEVICE and call(rets=None) == E.E_NO_DEVICE
        assert call(mask=p + 129) == E.E_NO_DEVICE                               # the mask may lie anywhere
        assert call(shift=0, nbins=1) == E.E_NO_DEVICE and call(shift=15, nbins=2) == E.E_NO_DEVICE
        assert call(shift=0, nbins=2048) == E.E_NO_DEVICE and call(esz=1, shift=7, nbins=2) == E.E_NO_DEVICE
        for H in (1, 2, 3, 1 << 40):
            assert call(H=H) == E.E_NO_DEVICE
        assert call(n=1 << 29, H=1) == E.E_NO_DEVICE and call(n=1 << 40, H=0) == E.E_NO_DEVICE     # exactly 2^40 entries; one histogram


SHAPES = [
    # (esz, D, chunk_len, n): whole rows and short last chunks (one ending mid-row), R % 8 != 0 and R < 8
    (1, 3, 3 * 33, 3 * 33 * 4 + 3 * 14),
    (2, 5, 5 * 21, 5 * 21 * 3 + 5 * 4 + 2),
    (1, 1, 13, 13 * 5 + 6),
    (2, 8, 8 * 64, 8 * 64 * 3),
    (1, 7, 7 * 5, 7 * 5 * 6 + 7),
]


def binnings(rng, esz, D):
    """(shift, nbins, lo): full resolution / the default shift, a number of bins that is no power of two, a random lo with wrap-around, one bin"""
    W = 8 * esz
    top = 1 << W
    return [(W - 8, 256, None), (hm.default_shift(esz, 64), 64, None), (W - 5, 19, None),
            (W - 6, 37, rng.integers(0, top, D)), (0, 100, rng.integers(0, top, D)), (W - 1, 1, None), (0, 1, rng.integers(0, top, D))]


@pytest.mark.parametrize("esz,D,chunk_len,n", SHAPES)
def test_model_equals_brute_force(esz, D, chunk_len, n):
    rng = np.random.default_rng(n + D)
    x = rng.integers(0, 1 << (8 * esz), n).astype(np.uint8 if esz == 1 else np.uint16)
    R, MB = fm.geometry(chunk_len, D)
    nchunks = -(-n // chunk_len)
    nrows = sum(ne // D for ne in fm.chunk_counts(n, chunk_len))
    for p in (None, 0.0, 0.3, 1.0):
        mask = None if p is None else random_mask(rng, nchunks, MB, p)     # bits of rows that do not exist are set too: they are ignored
        for shift, nbins, lo in binnings(rng, esz, D):
            for H in (0, 1, 2):
                got = hm.histogram_rows(x, chunk_len, D, mask, lo, shift, nbins, H)
                assert got.dtype == np.uint64 and got.shape == (-(-nchunks // H) if H else 1, D, nbins)
                assert np.array_equal(got, hm.histogram_rows_brute(x, chunk_len, D, mask, lo, shift, nbins, H)), (p, shift, nbins, H)
            if p in (None, 1.0) and lo is None and nbins << shift == 1 << (8 * esz):
                assert np.all(got.sum(axis=(0, 2)) == nrows)                 # the bins cover the range: every sample of every row
            if p == 0.0:
                assert not got.any()
    # np.bincount on the values themselves: full resolution, every row, one histogram
    full = hm.histogram_rows(x, chunk_len, D, None, None, 0, min(1 << (8 * esz), 65536))
    v = hm.selected_values(x, chunk_len, D)
    for d in range(D):
        assert np.array_equal(full[0, d], np.bincount(v[:, d], minlength=full.shape[2]))


def test_default_shift():
    assert [hm.default_shift(1, b) for b in (256, 255, 129, 128, 2, 1)] == [0, 0, 0, 1, 7, 7]      # (one bin: shift < W still holds)
    assert [hm.default_shift(2, b) for b in (65536, 256, 200, 16)] == [0, 8, 8, 12]


@pytest.mark.parametrize("esz,D,chunk_len,n", SHAPES)
def test_quantile_model_equals_sort(esz, D, chunk_len, n):
    rng = np.random.default_rng(n + 7)
    top = 1 << (8 * esz)
    x = (rng.integers(0, top, n) if D % 2 else np.clip(rng.normal(top / 2, top / 16, n), 0, top - 1)).astype(np.uint8 if esz == 1 else np.uint16)
    R, MB = fm.geometry(chunk_len, D)
    nchunks = -(-n // chunk_len)
    q = [0, 0.01, 0.25, 0.5, 0.99, 1]
    for p in (None, 0.3):
        mask = None if p is None else random_mask(rng, nchunks, MB, p)
        want = hm.quantiles(x, chunk_len, D, q, mask)
        v = hm.selected_values(x, chunk_len, D, mask)
        for i, qi in enumerate(q):
            for d in range(D):
                assert want[i, d] == np.sort(v[:, d])[max(int(np.ceil(qi * v.shape[0])), 1) - 1]
        assert np.array_equal(want[0], v.min(axis=0)) and np.array_equal(want[-1], v.max(axis=0))
        full = hm.histogram_rows(x, chunk_len, D, mask, None, 0, top)[0]
        assert np.array_equal(hm.quantiles_from_histogram(full, q), want.astype(np.int64))
    with pytest.raises(ValueError):
        hm.quantiles(x, chunk_len, D, q, np.zeros((nchunks, MB), np.uint8))


@pytest.fixture(scope="module")
def plan():
    planner.available()

    def ask(**fields):
        q = dict(codec=1, nchunks=4096, q=Q_HISTOGRAM)
        q.update(fields)
        nbins = q.pop("nbins", 256)
        if q["q"] == Q_HISTOGRAM:                # the table: D x nbins counters, a row adds at most 1 to one
            q.update(table_entries=q["D"] * nbins, table_row_max=1)
        return planner.split(planner.ask("decode", **q))
    return ask


def test_planner_edges(plan):
    # where the windowed query goes to decode_fast.h, so does the mode -- if the table fits the launch's LDS behind the groups' carves
    fast = [(1, 16, 16 * 512), (2, 8, 5120), (2, 24, 24 * 200), (1, 8, 4096), (2, 4, 4096), (1, 24, 24 * 200), (2, 5, 5 * 1024), (2, 3, 3000)]
    for esz, D, cl in fast:
        for codec in (0, 1):
            assert plan(esz=esz, D=D, chunk_len=cl, codec=codec, q=Q_WINDOW)[0] == "dec_fast", (esz, D, cl)
            fam, f = plan(esz=esz, D=D, chunk_len=cl, codec=codec)
            carve = plan(esz=esz, D=D, chunk_len=cl, codec=codec, q=Q_WINDOW)[1]["lds"]
            assert fam == "dec_fast" and f["table_off"] == carve and f["lds"] == carve + 4 * D * 256 and f["wg_chunks"] > 0, (esz, D, cl)
        fam, f = plan(esz=esz, D=D, chunk_len=cl, no_fast=1)
        assert fam == "dec_generic" and f["table_off"] == 0 and f["lds"] == 4 * D * 256, (esz, D, cl)
    # the LDS-budget edge: the carve + 4 D nbins <= 80 KB, one bin either side (uint16 x 8: the largest table is at the cap itself)
    seen = set()
    for esz, D, cl in [(2, 8, 5120), (1, 16, 16 * 512), (2, 24, 24 * 200), (1, 80, 10240), (2, 128, 128 * 80), (1, 256, 256 * 80)]:
        carve = plan(esz=esz, D=D, chunk_len=cl, q=Q_WINDOW)[1]["lds"]
        assert plan(esz=esz, D=D, chunk_len=cl, q=Q_WINDOW)[0] == "dec_fast"
        edge = (FAST_LDS_BUDGET - carve) // (4 * D) if carve <= FAST_LDS_BUDGET else 0      # the most bins decode_fast.h takes
        seen.add(0 if edge == 0 else 1 if edge < CAP // D else 2)
        for nbins in ({1, min(edge, CAP // D)} if edge >= 1 else ()):
            fam, f = plan(esz=esz, D=D, chunk_len=cl, nbins=nbins)
            assert fam == "dec_fast" and f["lds"] == carve + 4 * D * nbins <= FAST_LDS_BUDGET, (esz, D, nbins)
        if 1 <= edge + 1 <= CAP // D:
            fam, f = plan(esz=esz, D=D, chunk_len=cl, nbins=edge + 1)
            assert fam == "dec_generic" and f["lds"] == 4 * D * (edge + 1) and f["table_off"] == 0, (esz, D, edge)
    assert plan(esz=2, D=8, chunk_len=5120, nbins=2048)[0] == "dec_generic"      # the cap at uint16 x 8: 64 KB of table
    assert seen == {0, 1}                                                        # a carve above the budget; an edge below the cap (every carve is above 16 KB)
    # the low-dimension layouts: decode_uni.h serves the windowed query and is not taught this mode
    for esz, D, cl in [(1, 1, 1024), (2, 1, 1024), (1, 2, 2048), (2, 2, 2048), (1, 3, 3000), (1, 4, 4096)]:
        assert plan(esz=esz, D=D, chunk_len=cl, q=Q_WINDOW)[0] == "dec_uni", (esz, D, cl)
        assert plan(esz=esz, D=D, chunk_len=cl)[0] == "dec_generic", (esz, D, cl)
        assert plan(esz=esz, D=D, chunk_len=cl, no_fast=1)[0] == "dec_generic", (esz, D, cl)
    # everything else the windowed query leaves to the generic kernel
    for esz, D, cl in [(2, 300, 9600), (1, 512, 512 * 16), (2, 33, 33 * 64), (1, 5, 5 * 1024), (1, 33, 33 * 128), (2, 8, 8 * 13)]:
        for general in (0, 1):
            assert plan(esz=esz, D=D, chunk_len=cl, general=general, q=Q_WINDOW)[0] == "dec_generic", (esz, D, cl, general)
            assert plan(esz=esz, D=D, chunk_len=cl, general=general, nbins=16)[0] == "dec_generic", (esz, D, cl, general)
    for esz, D, cl in [(1, 4, 4096), (2, 2, 2048), (1, 1, 1024)]:                # general layout asked for on a low-dimension shape
        assert plan(esz=esz, D=D, chunk_len=cl, general=1)[0] == plan(esz=esz, D=D, chunk_len=cl, general=1, q=Q_WINDOW)[0]
    # the mode never reaches the small-batch, block-parallel or univariate kernels, whatever the batch size
    for nchunks in (1, 64, 2048, 2049, 131072):
        assert plan(esz=2, D=8, chunk_len=5120, nchunks=nchunks)[0] == "dec_fast"
        assert plan(esz=1, D=1, chunk_len=1024, nchunks=nchunks, codec=0)[0] == "dec_generic"
    # the chunks a workgroup counts in its table: 256 lanes / the lanes of a chunk (x the chunks a group decodes), and none where
    # their rows could wrap a 32-bit counter
    assert plan(esz=2, D=8, chunk_len=5120)[1]["wg_chunks"] == 32
    assert plan(esz=2, D=8, chunk_len=5120, chunks_per_group=4)[1]["wg_chunks"] == 128
    assert plan(esz=2, D=8, chunk_len=5120, no_fast=1)[1]["wg_chunks"] == 32
    assert plan(esz=1, D=1, chunk_len=1024)[1]["wg_chunks"] == 256
    assert plan(esz=1, D=1, chunk_len=(1 << 24) - 1)[1]["wg_chunks"] == 256       # 256 x (2^24 - 1) rows < 2^32
    assert plan(esz=1, D=1, chunk_len=1 << 24)[1]["wg_chunks"] == 0               # 2^32 rows: one too many
    assert plan(esz=2, D=8, chunk_len=1 << 30, nchunks=8)[1]["wg_chunks"] == 0    # 32 chunks of 2^27 rows
    assert plan(esz=2, D=8, chunk_len=1 << 30, nchunks=8, no_fast=1)[1]["wg_chunks"] == 0
    # the other modes' plans are what they were
    assert plan(esz=1, D=1, chunk_len=1024, q=5)[0] == "dec_uni" and plan(esz=1, D=1, chunk_len=1024, q=6)[0] == "dec_generic"
    assert plan(esz=2, D=8, chunk_len=5120, q=Q_AGGREGATE) == ("dec_fast", dict(plan(esz=2, D=8, chunk_len=5120, q=Q_WINDOW)[1]))
    assert plan(esz=2, D=8, chunk_len=5120, q=Q_WINDOW)[1]["table_off"] == 0 == plan(esz=2, D=8, chunk_len=5120, q=Q_WINDOW)[1]["wg_chunks"]
