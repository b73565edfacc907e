"""CPU tier of cumulative rows (sprintz_mi355x_cumulative_rows, ChunkedCodec.cumulative_rows): the symbols and their bindings are there, every
validation return comes before the device is touched, the numpy model the GPU tier compares with (tests/cumulative_model.py) equals a
brute-force loop on random and adversarial columns, keeps its carry contract wherever a batch is cut and wraps its sum modulo 2^64,
rowops' helpers follow it, and the planner (sprintz_amd/csrc/plan.h, built with g++: tests/plan_probe.cpp, asked with q=17 out_esz=...)
sends the mode to decode_fast.h for rows of whole 16-byte pieces with aligned outputs and to the generic kernel otherwise."""
import os

import numpy as np
import pytest

import cumulative_model as cm
import planner
import rolling_model as rm
from fixtures import buf_fixture, lib  # noqa: F401  (fixtures)
from rowdata import FLOAT_FAST_SHAPES as FAST_SHAPES, GENERIC_SHAPES, RAGGED_SHAPES

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = {1: np.uint8, 2: np.uint16}
Q_CUMULATIVE = 17                                         # geom.h: kQueryCumulative


buf = buf_fixture(32768)


def test_symbol_and_binding(lib):
    for name in ("sprintz_mi355x_cumulative_rows", "sprintz_mi355x_cumulative_tmp_bytes"):
        assert name in lib.EXPORTED_SYMBOLS and hasattr(lib.lib, name)
    assert len(lib.cumulative_rows.argtypes) == 18 and len(lib.cumulative_tmp_bytes.argtypes) == 2
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "size_t sprintz_mi355x_cumulative_tmp_bytes(uint64_t nchunks, uint16_t ndims);" in hdr
    assert "int sprintz_mi355x_cumulative_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    assert "uint32_t chunk_len, uint16_t ndims, uint32_t ops, int sum_bytes /* 4 or 8 */, uint32_t flags," in hdr
    assert "void* d_min, void* d_max, void* d_sum, const uint64_t* d_carry_in, uint64_t* d_carry_out," in hdr
    assert "void* d_tmp, int64_t* d_rets, void* hip_stream);" in hdr
    assert (lib.CUM_MIN, lib.CUM_MAX, lib.CUM_SUM) == (cm.MIN, cm.MAX, cm.SUM) == (1, 2, 4)
    for name, v in (("SPRINTZ_CUM_MIN", "1u"), ("SPRINTZ_CUM_MAX", "2u"), ("SPRINTZ_CUM_SUM", "4u")):
        assert f"#define {name}" in hdr and hdr.split(f"#define {name}")[1].split()[0] == v
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    geom = open(os.path.join(os.path.dirname(HERE), "sprintz_amd", "csrc", "geom.h")).read()
    assert f"kQueryCumulative = {Q_CUMULATIVE};" in geom
    assert f"kCumScanChunks = {cm.SCAN_CHUNKS};" in geom and "kCumScanTile = (uint32_t)kThreads * kCumScanChunks;" in geom
    from sprintz_amd import ChunkedCodec
    assert callable(ChunkedCodec.cumulative_rows)


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=8 * 640, D=8, ops=7, sb=8, flags=0, mn=p + 2048, mx=p + 4096, sm=p + 6144,
                cin=p + 8192, cout=p + 10240, tmp=p + 12288, rets=p + 16384)

    def call(**kw):
        a = dict(good, **kw)
        return lib.cumulative_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["ops"], a["sb"], a["flags"],
                                   a["mn"], a["mx"], a["sm"], a["cin"], a["cout"], a["tmp"], a["rets"], None)

    def refused(code, **kw):
        assert call(**kw) == code, kw
        assert "cumulative_rows" in lib.last_error(), (kw, lib.last_error())

    refused(E.E_INVALID, cl=8 * 640 + 1)                                         # bad geometry: chunk_len % ndims != 0
    refused(E.E_INVALID, D=7)
    refused(E.E_INVALID, cl=0)
    refused(E.E_INVALID, cl=(1 << 30) + 8)
    refused(E.E_INVALID, flags=2)                                                # unknown flag
    refused(E.E_INVALID, flags=4)
    for ops in (0, 8, 15):
        refused(E.E_INVALID, ops=ops)
    for k, bit in (("mn", 1), ("mx", 2), ("sm", 4)):
        refused(E.E_INVALID, **{k: None})                                        # an op without its output
        refused(E.E_INVALID, ops=7 & ~bit)                                       # an output without its op
    for sb in (0, 1, 2, 3, 5, 16, -8):
        refused(E.E_INVALID, sb=sb)
    refused(E.E_INVALID, sb=2, ops=3, sm=None)                                   # (checked whatever ops holds)
    refused(E.E_INVALID, mn=p + 2049)                                            # misaligned: min / max to the element size
    refused(E.E_INVALID, mx=p + 4097)
    refused(E.E_INVALID, sm=p + 6148)                                            # the sum to sum_bytes
    refused(E.E_INVALID, sm=p + 6146, sb=4)
    refused(E.E_INVALID, cin=p + 8196)                                           # the carries and rets to 8
    refused(E.E_INVALID, cout=p + 10244)
    refused(E.E_INVALID, rets=p + 16388)
    refused(E.E_INVALID, tmp=p + 12296)                                          # the scratch to 16
    refused(E.E_INVALID, tmp=None)                                               # more than one chunk: the scratch
    for k in ("comp", "offs"):
        refused(E.E_INVALID, **{k: None})
    assert call(D=0) == E.E_INVALID and call(codec=9) == E.E_INVALID and call(esz=3) == E.E_INVALID
    refused(E.E_UNSUPPORTED, D=513, cl=513 * 64)                                 # more than 512 columns
    for codec in (2, 3):
        refused(E.E_UNSUPPORTED, codec=codec)                                    # the non-RLE codecs
    assert call(n=0, cout=None) == 0                                             # nothing to do: returns 0, launches nothing
    assert call(n=0, cout=None, tmp=None, cin=None, rets=None) == 0
    import torch
    if not torch.cuda.is_available():
        assert call() == E.E_NO_DEVICE
        assert call(n=0) == E.E_NO_DEVICE                                        # carry_out takes the seeds: one tiny launch
        assert call(n=1, tmp=None, rets=None, cin=None, cout=None) == E.E_NO_DEVICE      # one chunk needs no scratch
        for ops in cm.SUBSETS:
            outs = {k: (good[k] if ops & bit else None) for k, bit in (("mn", 1), ("mx", 2), ("sm", 4))}
            assert call(ops=ops, **outs) == E.E_NO_DEVICE, ops
        assert call(flags=1) == E.E_NO_DEVICE and call(mn=p + 2050, sm=p + 6148, sb=4) == E.E_NO_DEVICE
        assert call(esz=1, mn=p + 2049, mx=p + 4097) == E.E_NO_DEVICE


# ------------------------------------------------------------------ the model

def columns(name, G, D, esz, rng):
    top = (1 << (8 * esz)) - 1
    r = np.arange(G, dtype=np.int64)[:, None] + np.arange(D, dtype=np.int64)[None, :] * 3
    if name == "constant":
        m = np.full((G, D), 0xA5 if esz == 1 else 0x1234, np.int64) + np.arange(D)[None, :]
    elif name == "zeros":
        m = np.zeros((G, D), np.int64)
    elif name == "ones":
        m = np.full((G, D), top, np.int64)
    elif name == "falling":
        m = top - r
    elif name == "rising":
        m = r
    else:
        m = rng.integers(0, top + 1, (G, D))
    assert m.min() >= 0 and m.max() <= top
    return m.astype(DTYPES[esz]).reshape(-1)


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("name", ["random", "constant", "zeros", "ones", "falling", "rising"])
def test_model_equals_brute_force(esz, name):
    rng = np.random.default_rng(esz)
    top = (1 << (8 * esz)) - 1
    for D, G, cut in ((1, 61, 0), (3, 50, 1), (8, 40, 5), (5, 150, 0)):
        x = columns(name, G, D, esz, rng)[:G * D - cut]                   # cut: a ragged tail, the last row partial
        for carry in (None, np.stack([rng.integers(0, top + 1, D), rng.integers(0, top + 1, D), rng.integers(0, 1 << 63, D)]).astype(np.uint64)):
            (got, left), (want, wleft) = cm.cumulative(x, D, carry), cm.brute(x, D, carry)
            for k in ("min", "max", "sum"):
                assert got[k].dtype == want[k].dtype and got[k].size == x.size and np.array_equal(got[k], want[k]), (name, D, k)
            assert left.dtype == np.uint64 and np.array_equal(left, wleft), (name, D)
        got, _ = cm.cumulative(x, D)
        g, d = np.arange(x.size) // D, np.arange(x.size) % D
        if name == "falling":                                              # the minimum is the newest row, the maximum the first
            assert np.array_equal(got["min"], x) and np.array_equal(got["max"], x[d])
        if name == "rising":
            assert np.array_equal(got["max"], x) and np.array_equal(got["min"], x[d])
        if name in ("constant", "ones"):
            assert np.array_equal(got["min"], x) and np.array_equal(got["max"], x) and np.array_equal(got["sum"], x.astype(np.uint64) * (g + 1).astype(np.uint64))
        for ops in cm.SUBSETS:                                             # a subset of the ops: those outputs alone, the others' seeds passed through
            sub, left = cm.cumulative(x, D, None, ops)
            assert tuple(sub) == cm.names(ops) and all(np.array_equal(sub[k], got[k]) for k in sub)
            full = cm.cumulative(x, D)[1]
            for i, bit in enumerate((1, 2, 4)):
                assert np.array_equal(left[i], full[i] if ops & bit else cm.identity(D, esz)[i])


@pytest.mark.parametrize("esz,D,chunk_len,n", RAGGED_SHAPES)
def test_model_on_the_ragged_shapes(esz, D, chunk_len, n):
    rng = np.random.default_rng(n)
    x = rng.integers(0, 1 << (8 * esz), n).astype(DTYPES[esz])
    (got, left), (want, wleft) = cm.cumulative(x, D), cm.brute(x, D)
    assert all(np.array_equal(got[k], want[k]) for k in want) and np.array_equal(left, wleft)
    # a damaged chunk counts as absent: everything outside it equals the model of the batch without it
    R = chunk_len // D
    nchunks = -(-n // chunk_len)
    for bad in range(nchunks):
        rest = np.concatenate([x[:bad * chunk_len], x[(bad + 1) * chunk_len:]])
        (got, left), (want, wleft) = cm.cumulative(x, D, None, 7, chunk_len, (bad,)), cm.cumulative(rest, D)
        keep = np.arange(n) // chunk_len != bad
        if bad + 1 < nchunks or n % chunk_len == 0 or (n % chunk_len) % D == 0:      # (removing a last chunk that ends mid-row leaves whole rows: the same columns)
            assert all(np.array_equal(got[k][keep], want[k]) for k in want), (bad, R)
            assert np.array_equal(left, wleft)


@pytest.mark.parametrize("esz,D,R", [(2, 8, 24), (1, 3, 16), (2, 1, 40), (1, 7, 5)])
def test_model_carry_contract(esz, D, R):
    """cut anywhere -- at chunk seams, inside a chunk, at row 0 and behind the last row (an empty batch) -- and chain: the result is one call's"""
    rng = np.random.default_rng(D * R)
    G = 5 * R + 3
    x = rng.integers(0, 1 << (8 * esz), G * D - (D // 2)).astype(DTYPES[esz])
    seed = np.stack([rng.integers(0, 1 << (8 * esz), D).astype(np.uint64), rng.integers(0, 1 << (8 * esz), D).astype(np.uint64), rng.integers(0, 1 << 64, D, dtype=np.uint64)])
    for carry in (None, seed):
        one, left = cm.cumulative(x, D, carry)
        for cuts in ([R], [2 * R], [R - 1], [R + 1], [1], [G - 1], [0], [G], [7, 7, 2 * R + 5], [R, 2 * R, 3 * R, 4 * R], sorted(rng.integers(0, G + 1, 6).tolist())):
            got, gleft = cm.chained(x, D, cuts, carry)
            assert all(np.array_equal(got[k], one[k]) for k in one), cuts
            assert np.array_equal(gleft, left), cuts
    empty, left = cm.cumulative(x[:0], D, seed)
    assert all(v.size == 0 for v in empty.values()) and np.array_equal(left, cm.seeds(seed, D, esz))


def test_model_sum_wraps():
    """the sum is modulo 2^64, its int32 form the low 32 bits: seeds just below 2^32, at 2^40 and just below 2^63 and 2^64"""
    D = 5
    x = np.full(64 * D, 65535, np.uint16)
    seed = cm.identity(D, 2)
    seed[2] = np.array([(1 << 32) - 5, 1 << 40, (1 << 63) - 1, (1 << 64) - 3, 0], dtype=np.uint64)
    got, left = cm.cumulative(x, D, seed)
    g = np.arange(x.size) // D
    for d in range(D):
        want = [(int(seed[2][d]) + 65535 * (r + 1)) & cm.M64 for r in range(64)]
        assert got["sum"][d::D].tolist() == want
        assert cm.int64(got["sum"])[d::D].tolist() == [w - (1 << 64) if w >> 63 else w for w in want]
        assert cm.low32(got["sum"])[d::D].tolist() == [(w & 0xFFFFFFFF) - (1 << 32) if (w >> 31) & 1 else w & 0xFFFFFFFF for w in want]
        assert int(left[2][d]) == want[-1]
    assert cm.int64(got["sum"])[2] < 0 < int(seed[2][2]) and got["sum"][3] < seed[2][3]      # across 2^63, across 2^64
    assert cm.low32(got["sum"])[0] == 65535 - 5                                               # across 2^32
    assert np.array_equal(cm.mean(got["sum"], D, 10)[4::D], 65535.0 * (np.arange(64) + 1) / (np.arange(64) + 11))
    assert g.max() == 63


# ------------------------------------------------------------------ the scratch, rowops

def test_tmp_bytes(lib):
    from sprintz_amd import rowops
    assert lib.cumulative_tmp_bytes(0, 8) == lib.cumulative_tmp_bytes(1, 8) == 0 == rowops.cumulative_tmp_bytes(1, 8)
    for D in (1, 3, 8, 80, 512):
        last = 0
        for n in list(range(2, 40)) + [cm.SCAN_TILE - 1, cm.SCAN_TILE, 2 * cm.SCAN_TILE + 1, 131072]:
            b = lib.cumulative_tmp_bytes(n, D)
            assert b == cm.tmp_bytes(n, D) == rowops.cumulative_tmp_bytes(n, D) and b % 16 == 0 and b > last, (n, D)
            lay = cm.tmp_layout(n, D)
            assert all(lay[k] % 16 == 0 for k in lay) and lay["rets"] >= n * D * 24 and lay["sum"] - lay["rets"] >= n * 8
            assert lay["min"] - lay["sum"] >= n * D * 8 and lay["max"] - lay["min"] >= n * D * 2 and lay["bytes"] - lay["max"] >= n * D * 2
            last = b
    for n in (2, 5, 1000):                                                      # monotone in the columns too
        sizes = [lib.cumulative_tmp_bytes(n, D) for D in range(1, 513)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)


def test_rowops_helpers():
    import torch
    from sprintz_amd import rowops
    assert rowops.CUMULATIVE_OPS == ("min", "max", "sum", "mean")
    for esz in (1, 2):
        c = rowops.cumulative_carry(5, esz)
        assert c.rows == 0 and c.table.dtype == torch.int64 and np.array_equal(c.table.numpy().view(np.uint64), cm.identity(5, esz))
        assert rowops.check_carry(c, 5, c.table.device) is c
        for bad in (None, c.table, rowops.CumulativeCarry(c.table[:, :4]), rowops.CumulativeCarry(c.table.to(torch.int32)), rowops.CumulativeCarry(c.table.t())):
            with pytest.raises(ValueError):
                rowops.check_carry(bad, 5, c.table.device)
    rng = np.random.default_rng(3)
    D, G = 5, 90
    x = rng.integers(0, 65536, G * D).astype(np.uint16)
    total = cm.cumulative(x, D)[0]["sum"]
    for before in (0, 77):
        got = rowops.cumulative_mean(torch.from_numpy(cm.int64(total)).view(G, D), before)
        assert got.dtype == torch.float64 and np.array_equal(got.numpy().reshape(-1), cm.mean(total, D, before))
    assert got[0, 0].item() == float(x[0]) / 78


# ------------------------------------------------------------------ the planner

@pytest.fixture(scope="module")
def plan():
    planner.available()
    return lambda **fields: planner.ask("decode", q=Q_CUMULATIVE, **fields)


def named_chunk_len(D):
    """48 rows: three groups of 16, and long enough for decode_fast.h's read-ahead ring on every shape it serves (37 .. 48 rows)"""
    return D * 48


@pytest.mark.parametrize("esz,D", FAST_SHAPES + GENERIC_SHAPES)
def test_planner_family(plan, esz, D):
    """the family for every named shape: decode_fast.h for rows of whole 16-byte pieces on a one-column-a-lane mapping (8 .. 64 columns) with
    aligned outputs, the plain decode's carve as its LDS; the generic kernel, without LDS, for everything else -- the low-dim shapes,
    NO_FAST, a misaligned output"""
    chunk_len = named_chunk_len(D)
    seen = set()
    for general in (0, 1):
        dp = rm.lanes(esz, D, general)
        fdp, _, carve = rm.fast_map(esz, D)
        for osz in (esz, 4, 8):                                                  # without the sum, with the int32 and with the int64 one
            for no_fast in (0, 1):
                for cpg in (1, 3):
                    for out_lo in (0, 8):
                        got = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=7, codec=1, out_esz=osz, general=general, no_fast=no_fast,
                                   chunks_per_group=cpg, out_lo=out_lo)
                        if cm.fast_takes(esz, D, chunk_len, general, no_fast, out_lo, osz):
                            assert got.get("family") == "dec_fast", got
                            assert got["lds_group_stride"] == carve and got["lds"] == carve * (rm.THREADS // fdp) and got["table_off"] == 0, got
                            assert got["dp"] == fdp and got["cpl"] == 1 and got["chunks_per_group"] == cpg and got["grid"] == -(--(-7 // cpg) * fdp // rm.THREADS), got
                        else:
                            assert got.get("family") == "dec_generic", got
                            assert got["lds"] == 0 and got["log2DP"] == dp.bit_length() - 1 and got["grid"] == -(-7 * dp // rm.THREADS) and got["vec_store"] == 0, got
                        seen.add(got["family"])
    fast = (esz, D) in ((2, 8), (2, 16), (2, 24), (2, 64), (1, 16))
    assert fast == ((esz, D) in FAST_SHAPES and D * esz <= 128 and D <= 64)      # (the named shapes of one column a lane)
    assert seen == ({"dec_fast", "dec_generic"} if fast else {"dec_generic"})


def test_planner_fast_for_the_fast_shapes_with_aligned_outputs(plan):
    for esz, D in FAST_SHAPES:
        got = plan(esz=esz, D=D, chunk_len=named_chunk_len(D), nchunks=9, codec=0, out_esz=8)
        assert got.get("family") == ("dec_fast" if rm.fast_map(esz, D)[1] == 1 else "dec_generic"), (esz, D, got)       # (two and four columns a lane stay generic)
    for esz, D in GENERIC_SHAPES + [(1, 2), (1, 3), (2, 2)]:
        for general in (0, 1):
            assert plan(esz=esz, D=D, chunk_len=named_chunk_len(D), nchunks=9, codec=0, out_esz=8, general=general).get("family") == "dec_generic"


@pytest.mark.parametrize("esz,D", [(2, 8), (1, 16), (2, 64)])
def test_planner_hands_over_at_the_descriptor_reach(plan, esz, D):
    """both sides of chunk_len x out_esz x 4096 < 0xf0000000: the widest output element counts, so the int64 sum leaves decode_fast.h at an
    eighth of the chunk length the minimum does"""
    for osz in (esz, 4, 8):
        rows = (0xf0000000 // 4096 // osz) // D
        rows -= rows % 16
        while D * rows * osz * 4096 >= 0xf0000000:
            rows -= 16
        inside, beyond = D * rows, D * (rows + 16)
        assert inside * osz * 4096 < 0xf0000000 <= beyond * osz * 4096
        assert plan(esz=esz, D=D, chunk_len=inside, nchunks=3, codec=1, out_esz=osz).get("family") == "dec_fast"
        assert plan(esz=esz, D=D, chunk_len=beyond, nchunks=3, codec=1, out_esz=osz).get("family") == "dec_generic"
        if osz < 8:                                                              # the same chunk with a wider output: past the reach
            assert plan(esz=esz, D=D, chunk_len=inside, nchunks=3, codec=1, out_esz=8).get("family") == "dec_generic"


def test_planner_refuses_what_the_mode_does_not_take(plan):
    assert plan(esz=1, D=513, chunk_len=513 * 16, nchunks=3, codec=0, out_esz=8).get("error") == -4      # SPRINTZ_E_UNSUPPORTED
    for codec in (2, 3):
        got = plan(esz=1, D=8, chunk_len=8 * 64, nchunks=3, codec=codec, out_esz=8)
        assert got.get("error") == -4 and "cumulative_rows" in got["what"], got


def test_planner_leaves_the_other_modes_alone():
    """out_esz means nothing to the plain decode: its plan is the one it had"""
    planner.available()
    base = dict(esz=2, D=8, chunk_len=5120, nchunks=4096, codec=1)
    assert planner.ask("decode", **base) == planner.ask("decode", out_esz=8, **base)
    assert planner.ask("decode", **base)["family"] == "dec_fast"
