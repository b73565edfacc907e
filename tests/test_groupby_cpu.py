"""CPU tests of group-by rows (sprintz_mi355x_groupby_rows): the symbol and its binding are there, every validation return comes before
the device is touched and names the operation, the numpy model the GPU tier compares with (tests/groupby_model.py) equals brute force and
satisfies the identities that tie it to the column sums and to the histogram of the key column, and the planner (sprintz_amd/csrc/plan.h,
built with g++: tests/plan_probe.cpp) sends the mode to decode_fast.h where the windowed query goes AND the table fits the
launch's LDS next to the groups' carves, to the generic kernel otherwise -- never to decode_uni.h -- and gives a workgroup its 32-bit
table only where no sum can wrap."""
import os

import numpy as np
import pytest

import filter_model as fm
import groupby_model as gm
import histogram_model as hm
import planner
from fixtures import buf_fixture, lib, random_mask, refusals  # noqa: F401  (fixtures)
from planner import QUERY

HERE = os.path.dirname(os.path.abspath(__file__))
Q_WINDOW, Q_AGGREGATE, Q_HISTOGRAM, Q_GROUPBY = QUERY["window"], QUERY["aggregate"], QUERY["histogram"], QUERY["groupby"]
CAP = 16384
FAST_LDS_BUDGET = 80 * 1024           # geom.h: kHistFastLdsBudget


buf = buf_fixture(65536)


def test_symbol_and_binding(lib):
    assert "sprintz_mi355x_groupby_rows" in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.lib, "sprintz_mi355x_groupby_rows")
    assert len(lib.groupby_rows.argtypes) == 19
    assert (lib.GBY_COUNT, lib.GBY_SUM, lib.GBY_MAX_COUNTERS) == (1, 2, CAP)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_groupby_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    assert "uint32_t key_col, uint32_t key_lo, uint32_t shift, uint32_t nbins, uint64_t table_chunks," in hdr
    assert "uint32_t ops, uint32_t flags, uint64_t* d_count, uint64_t* d_sum, int64_t* d_rets, void* hip_stream);" in hdr
    assert "#define SPRINTZ_GBY_COUNT 1u" in hdr and "#define SPRINTZ_GBY_SUM   2u" in hdr
    assert "#define SPRINTZ_GBY_MAX_COUNTERS 16384u" in hdr
    assert "groupby_rows, SPRINTZ_GBY_*" in hdr                   # the ABI-history comment
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    from sprintz_amd import ChunkedCodec
    assert callable(ChunkedCodec.groupby_rows) and callable(ChunkedCodec.groupby_where)


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=5120, D=8, mask=p + 128, key=0, key_lo=0, shift=8, nbins=256, H=0, ops=3, flags=0,
                count=p + 2048, sum=p + 8192, rets=p + 32768)

    def call(**kw):
        a = dict(good, **kw)
        return lib.groupby_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["mask"], a["key"], a["key_lo"], a["shift"],
                                a["nbins"], a["H"], a["ops"], a["flags"], a["count"], a["sum"], a["rets"], None)

    invalid, unsupported = refusals(lib, call, "groupby_rows")

    invalid(cl=5121)                                                             # chunk_len % ndims != 0
    invalid(D=7)
    invalid(cl=0)                                                                # chunk_len outside 1..2^30
    invalid(cl=(1 << 30) + 8)
    for key in (8, 9, 512, 0xFFFFFFFF):                                          # key_col < D
        invalid(key=key)
    invalid(D=1, cl=1024, key=1)
    for key_lo in (1 << 16, (1 << 16) + 1, 0xFFFFFFFF):                          # key_lo < 2^W
        invalid(key_lo=key_lo)
    invalid(esz=1, shift=0, key_lo=256)
    for shift in (16, 17, 32, 0xFFFFFFFF):                                       # 0 <= shift < W
        invalid(shift=shift)
    for shift in (8, 9, 31):
        invalid(esz=1, shift=shift, nbins=1)
    invalid(nbins=0)                                                             # 1 <= nbins <= 2^(W - shift)
    invalid(nbins=257)                                                           # (shift 8 at 16 bits: 256 bins are the range)
    invalid(shift=15, nbins=3)
    invalid(esz=1, shift=0, nbins=257)
    invalid(esz=1, shift=4, nbins=17)
    invalid(ops=0)                                                               # ops == 0 or an unknown bit
    for ops in (4, 5, 7, 8, 0x80000001):
        invalid(ops=ops)
    invalid(count=None)                                                          # a selected output that is NULL
    invalid(sum=None)
    invalid(ops=1, count=None)
    invalid(ops=2, sum=None)
    for k in ("comp", "offs"):                                                   # NULL d_comp / d_offsets
        invalid(**{k: None})
    for off in (1, 2, 4):                                                        # d_count / d_sum / d_rets not aligned to 8 bytes
        invalid(count=p + 2048 + off)
        invalid(sum=p + 8192 + off)
        invalid(rets=p + 32768 + off)
    invalid(n=(1 << 29) + 1, H=1)                                                # more than 2^40 entries of d_sum: 2^29 + 1 tables of 256 x 8
    invalid(n=1 << 40, H=1)
    invalid(n=(1 << 40) + 1, H=2, D=512, cl=512 * 16, nbins=31, shift=11)
    invalid(flags=2)                                                             # unknown flag (GENERAL_LAYOUT = 1 is the only one)
    invalid(flags=3)
    assert call(D=0) == E.E_INVALID and call(codec=9) == E.E_INVALID and call(esz=3) == E.E_INVALID
    # the cap, both sides of 16384 = nbins x (D + 1) entries
    unsupported(D=8, shift=0, nbins=1821)                                        # 1821 x 9 = 16389
    unsupported(D=64, cl=64 * 16, shift=8, nbins=253)                            # (256 x 64 is the cap: 63 columns take 256 bins, 64 take 252)
    unsupported(esz=1, D=80, cl=80 * 16, shift=0, nbins=203)
    unsupported(D=512, cl=512 * 16, shift=8, nbins=32)
    unsupported(D=513, cl=513 * 16, nbins=1)                                     # more than 512 columns
    for codec in (2, 3):
        unsupported(codec=codec)                                                 # the non-RLE codecs
    unsupported(codec=4, esz=1, shift=0)
    assert call(n=0) == 0                                                        # nothing to do: returns 0, launches nothing
    assert call(n=0, mask=None, rets=None) == 0
    import torch
    if not torch.cuda.is_available():
        assert call() == E.E_NO_DEVICE
        assert call(D=8, shift=0, nbins=1820) == E.E_NO_DEVICE                   # 1820 x 9 = 16380: the most bins 8 columns take
        assert call(D=63, cl=63 * 16, shift=8, nbins=256) == E.E_NO_DEVICE       # exactly the cap
        assert call(D=64, cl=64 * 16, shift=8, nbins=252) == E.E_NO_DEVICE
        assert call(esz=1, D=80, cl=80 * 16, shift=0, nbins=202) == E.E_NO_DEVICE
        assert call(D=512, cl=512 * 16, shift=8, nbins=31, flags=1) == E.E_NO_DEVICE
        assert call(mask=None) == E.E_NO_DEVICE and call(rets=None) == E.E_NO_DEVICE
        assert call(mask=p + 129) == E.E_NO_DEVICE                               # the mask may lie anywhere
        assert call(ops=1, sum=None) == E.E_NO_DEVICE and call(ops=2, count=None) == E.E_NO_DEVICE      # an unselected output may be NULL ...
        assert call(ops=1, sum=p + 8193) == E.E_NO_DEVICE and call(ops=2, count=p + 2052) == E.E_NO_DEVICE   # ... or lie anywhere
        assert call(key=7) == E.E_NO_DEVICE and call(key_lo=65535) == E.E_NO_DEVICE and call(esz=1, shift=0, key_lo=255) == E.E_NO_DEVICE
        assert call(shift=0, nbins=1) == E.E_NO_DEVICE and call(shift=15, nbins=2) == E.E_NO_DEVICE
        assert call(esz=1, shift=7, nbins=2) == E.E_NO_DEVICE
        for H in (1, 2, 3, 1 << 40):
            assert call(H=H) == E.E_NO_DEVICE
        assert call(n=1 << 29, H=1) == E.E_NO_DEVICE and call(n=1 << 40, H=0) == E.E_NO_DEVICE     # exactly 2^40 entries; one table


SHAPES = [
    # (esz, D, chunk_len, n): whole rows and short last chunks (one ending mid-row), R % 8 != 0 and R < 8
    (1, 3, 3 * 33, 3 * 33 * 4 + 3 * 14),
    (2, 5, 5 * 21, 5 * 21 * 3 + 5 * 4 + 2),
    (1, 1, 13, 13 * 5 + 6),
    (2, 8, 8 * 64, 8 * 64 * 3),
    (1, 7, 7 * 5, 7 * 5 * 6 + 7),
]


def binnings(rng, esz):
    """(shift, nbins, key_lo): the bins that cover the range, a number of bins that is no power of two, a random key_lo with wrap-around
    under fewer bins than the range, full resolution around a random value, one bin"""
    W = 8 * esz
    top = 1 << W
    return [(W - 8, 256, 0), (gm.default_shift(esz, 64), 64, 0), (W - 5, 19, 0), (W - 6, 37, int(rng.integers(1, top))),
            (0, 100, int(rng.integers(1, top))), (W - 1, 1, 0), (0, 1, int(rng.integers(1, top)))]


@pytest.mark.parametrize("esz,D,chunk_len,n", SHAPES)
def test_model_equals_brute_force(esz, D, chunk_len, n):
    rng = np.random.default_rng(n + D)
    W = 8 * esz
    x = rng.integers(0, 1 << W, n).astype(np.uint8 if esz == 1 else np.uint16)
    R, MB = fm.geometry(chunk_len, D)
    nchunks = -(-n // chunk_len)
    lens = fm.chunk_counts(n, chunk_len)
    nrows = sum(ne // D for ne in lens)
    rows = np.concatenate([x[c * chunk_len:c * chunk_len + ne // D * D] for c, ne in enumerate(lens)]).reshape(-1, D).astype(np.uint64)
    for p in (None, 0.0, 0.3, 1.0):
        mask = None if p is None else random_mask(rng, nchunks, MB, p)     # bits of rows that do not exist are set too: they are ignored
        for key in sorted({0, D - 1, D // 2}):
            for shift, nbins, key_lo in binnings(rng, esz):
                for H in (0, 1, 2):
                    cnt, tot = gm.groupby_rows(x, chunk_len, D, key, mask, key_lo, shift, nbins, H)
                    assert cnt.dtype == tot.dtype == np.uint64
                    assert cnt.shape == (-(-nchunks // H) if H else 1, nbins) and tot.shape == cnt.shape + (D,)
                    bc, bt = gm.groupby_rows_brute(x, chunk_len, D, key, mask, key_lo, shift, nbins, H)
                    assert np.array_equal(cnt, bc) and np.array_equal(tot, bt), (p, key, shift, nbins, H)
                    # the count table is the histogram of the key column
                    lo = np.zeros(D, np.int64)
                    lo[key] = key_lo
                    assert np.array_equal(cnt, hm.histogram_rows(x, chunk_len, D, mask, lo, shift, nbins, H)[:, key, :])
                if p in (None, 1.0) and key_lo == 0 and nbins << shift == 1 << W:
                    # the bins cover the key's range and every row is selected: no row is dropped
                    assert int(cnt.sum()) == nrows
                    assert np.array_equal(tot.sum(axis=(0, 1)), rows.sum(axis=0))
                if p == 0.0:
                    assert not cnt.any() and not tot.any()
    m = gm.mean(*gm.groupby_rows(x, chunk_len, D, 0, None, 0, W - 3, 8, 0))
    cnt, tot = gm.groupby_rows(x, chunk_len, D, 0, None, 0, W - 3, 8, 0)
    assert m.shape == tot.shape and np.array_equal(np.isnan(m[..., 0]), cnt == 0)


def test_default_shift():
    assert [gm.default_shift(1, b) for b in (256, 255, 129, 128, 2, 1)] == [0, 0, 0, 1, 7, 7]      # (one bin: shift < W still holds)
    assert [gm.default_shift(2, b) for b in (65536, 256, 200, 16)] == [0, 8, 8, 12]


@pytest.fixture(scope="module")
def plan():
    planner.available()

    def ask(**fields):
        q = dict(codec=1, nchunks=4096, q=Q_GROUPBY)
        q.update(fields)
        nbins = q.pop("nbins", 256)
        if q["q"] == Q_GROUPBY:                  # the table: nbins x (D + 1) entries, a row adds at most 2^W - 1 to one
            q.update(table_entries=nbins * (q["D"] + 1), table_row_max=(1 << (8 * q["esz"])) - 1)
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
            assert fam == "dec_fast" and f["table_off"] == carve and f["lds"] == carve + 4 * 256 * (D + 1) and f["wg_chunks"] > 0, (esz, D, cl)
        fam, f = plan(esz=esz, D=D, chunk_len=cl, no_fast=1)
        assert fam == "dec_generic" and f["table_off"] == 0 and f["lds"] == 4 * 256 * (D + 1), (esz, D, cl)
    # the LDS-budget edge: the carve + 4 nbins (D + 1) <= 80 KB, one bin either side
    seen = set()
    for esz, D, cl in [(2, 8, 5120), (1, 16, 16 * 512), (2, 24, 24 * 200), (1, 80, 10240), (2, 128, 128 * 80), (1, 256, 256 * 80)]:
        carve = plan(esz=esz, D=D, chunk_len=cl, q=Q_WINDOW)[1]["lds"]
        assert plan(esz=esz, D=D, chunk_len=cl, q=Q_WINDOW)[0] == "dec_fast"
        most = CAP // (D + 1)                                                    # the most bins a call takes
        edge = (FAST_LDS_BUDGET - carve) // (4 * (D + 1)) if carve <= FAST_LDS_BUDGET else 0      # the most bins decode_fast.h takes
        seen.add(0 if edge == 0 else 1 if edge < most else 2)
        for nbins in ({1, min(edge, most)} if edge >= 1 else ()):
            fam, f = plan(esz=esz, D=D, chunk_len=cl, nbins=nbins)
            assert fam == "dec_fast" and f["table_off"] == carve and f["lds"] == carve + 4 * nbins * (D + 1) <= FAST_LDS_BUDGET, (esz, D, nbins)
        if 1 <= edge + 1 <= most:
            fam, f = plan(esz=esz, D=D, chunk_len=cl, nbins=edge + 1)
            assert fam == "dec_generic" and f["lds"] == 4 * (edge + 1) * (D + 1) and f["table_off"] == 0, (esz, D, edge)
    assert plan(esz=2, D=8, chunk_len=5120, nbins=1820)[0] == "dec_generic"      # the cap at uint16 x 8: 64 KB of table
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
    # the other modes' plans are what they were
    assert plan(esz=1, D=1, chunk_len=1024, q=5)[0] == "dec_uni" and plan(esz=1, D=1, chunk_len=1024, q=6)[0] == "dec_generic"
    assert plan(esz=2, D=8, chunk_len=5120, q=Q_AGGREGATE) == ("dec_fast", dict(plan(esz=2, D=8, chunk_len=5120, q=Q_WINDOW)[1]))
    assert plan(esz=2, D=8, chunk_len=5120, q=Q_HISTOGRAM)[1]["table_off"] == 0 == plan(esz=2, D=8, chunk_len=5120, q=Q_HISTOGRAM)[1]["wg_chunks"]
    assert plan(esz=2, D=8, chunk_len=5120, q=Q_WINDOW)[1]["table_off"] == 0 == plan(esz=2, D=8, chunk_len=5120, q=Q_WINDOW)[1]["wg_chunks"]


def test_planner_wrap_rule(plan):
    """a workgroup adds in a table of uint32: a sum takes at most 2^W - 1 a row, so the table is given only where
    wg_chunks x R x (2^W - 1) <= 2^32 - 1, and wg_chunks = 0 (every add goes to global memory) otherwise"""
    # the headline shape: uint16 x 8, 640 rows a chunk, 32 chunks a workgroup -- 32 x 640 x 65535 = 1 342 156 800 passes the rule;
    # four chunks a lane group (128 a workgroup) do not
    assert 32 * 640 * 65535 == 1342156800 <= 2**32 - 1 < 128 * 640 * 65535
    assert plan(esz=2, D=8, chunk_len=5120)[1]["wg_chunks"] == 32
    assert plan(esz=2, D=8, chunk_len=5120, codec=0)[1]["wg_chunks"] == 32
    assert plan(esz=2, D=8, chunk_len=5120, no_fast=1)[1]["wg_chunks"] == 32
    fam, f = plan(esz=2, D=8, chunk_len=5120, chunks_per_group=4)
    assert fam == "dec_fast" and f["wg_chunks"] == 0 and f["table_off"] > 0       # (the launch's LDS is what it was: the table is not used)
    assert plan(esz=2, D=8, chunk_len=5120, chunks_per_group=2)[1]["wg_chunks"] == 64      # 64 x 640 x 65535 = 2 684 313 600
    assert plan(esz=2, D=8, chunk_len=5120, chunks_per_group=3)[1]["wg_chunks"] == 96      # 96 x 640 x 65535 = 4 026 470 400
    assert 96 * 640 * 65535 <= 2**32 - 1
    # the exact edge at 16 bits: 65537 x 65535 = 2^32 - 1, so 65537 rows a workgroup are the most.  32 chunks a workgroup (uint16 x 8):
    # 2048 rows a chunk are 65536 rows, 2049 are 65568.  The GPU tier runs these two shapes on constant 0xFFFF data
    assert 65537 * 65535 == 2**32 - 1
    for kw in (dict(), dict(no_fast=1)):
        assert plan(esz=2, D=8, chunk_len=8 * 2048, **kw)[1]["wg_chunks"] == 32
        assert plan(esz=2, D=8, chunk_len=8 * 2049, **kw)[1]["wg_chunks"] == 0
        assert plan(esz=2, D=8, chunk_len=8 * 2056, **kw)[1]["wg_chunks"] == 0
    # one column, low-dimension layout: 256 chunks a workgroup, 256 rows a chunk are 65536 rows
    assert plan(esz=2, D=1, chunk_len=256)[1]["wg_chunks"] == 256
    assert plan(esz=2, D=1, chunk_len=257)[1]["wg_chunks"] == 0
    # the exact edge at 8 bits: 16843009 x 255 = 2^32 - 1.  32 chunks a workgroup (uint8 x 8 under NO_FAST): 526344 rows a chunk are
    # 16843008 rows; one more row a chunk is too many
    assert 16843009 * 255 == 2**32 - 1 and 32 * 526344 == 16843008
    assert plan(esz=1, D=8, chunk_len=8 * 526344, no_fast=1, nchunks=64)[1]["wg_chunks"] == 32
    assert plan(esz=1, D=8, chunk_len=8 * 526345, no_fast=1, nchunks=64)[1]["wg_chunks"] == 0
    # one column at 8 bits: 256 chunks of 65793 rows are 16843008 rows
    assert plan(esz=1, D=1, chunk_len=65793, codec=0)[1]["wg_chunks"] == 256
    assert plan(esz=1, D=1, chunk_len=65794, codec=0)[1]["wg_chunks"] == 0
    # the largest chunks there are
    assert plan(esz=2, D=8, chunk_len=1 << 30, nchunks=8)[1]["wg_chunks"] == 0
    assert plan(esz=1, D=1, chunk_len=1 << 30, nchunks=8, no_fast=1)[1]["wg_chunks"] == 0


def test_planner_cap(plan):
    """nbins x (D + 1) at SPRINTZ_GBY_MAX_COUNTERS: the largest tables a call can ask for are planned (the entry point refuses more)"""
    for esz, D, cl, nbins in [(2, 63, 63 * 64, 256), (2, 8, 5120, 1820), (1, 511, 511 * 16, 32), (2, 1, 1024, 8192), (1, 3, 3000, 256)]:
        assert nbins * (D + 1) <= CAP < (nbins + 1) * (D + 1) or nbins == 1 << (8 * esz)
        fam, f = plan(esz=esz, D=D, chunk_len=cl, nbins=nbins)
        assert fam in ("dec_fast", "dec_generic") and f["lds"] >= 4 * nbins * (D + 1), (esz, D, nbins)
        if fam == "dec_generic":
            assert f["lds"] == 4 * nbins * (D + 1) <= 4 * CAP and f["table_off"] == 0
