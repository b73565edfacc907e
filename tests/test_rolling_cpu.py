"""CPU tier of rolling rows (sprintz_mi355x_rolling_rows, ChunkedCodec.rolling_rows): the symbol and its binding are there, every validation
return comes before the device is touched, the numpy model the GPU tier compares with (tests/rolling_model.py) equals a brute-force loop
on random and adversarial columns, rowops' helpers follow it, and the planner (sprintz_amd/csrc/plan.h, built with g++:
tests/plan_probe.cpp, asked with q=15 rows=W out_esz=...) sends the mode to the generic kernel with the rings as its LDS and refuses a
window whose rings do not fit -- both sides of that edge, computed here from geom.h's formulas restated in Python."""
import os

import numpy as np
import pytest

import planner
import rolling_model as rm
from fixtures import buf_fixture, lib  # noqa: F401  (fixtures)
from rowdata import FLOAT_FAST_SHAPES as FAST_SHAPES, GENERIC_SHAPES, RAGGED_SHAPES

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = {1: np.uint8, 2: np.uint16}
Q_ROLLING = 15                                            # geom.h: kQueryRolling


buf = buf_fixture(16384)


def test_symbol_and_binding(lib):
    assert "sprintz_mi355x_rolling_rows" in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.lib, "sprintz_mi355x_rolling_rows")
    assert len(lib.rolling_rows.argtypes) == 16
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_rolling_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    assert "uint32_t chunk_len, uint16_t ndims, uint32_t window_rows, uint32_t ops, uint32_t flags," in hdr
    assert "void* d_min, void* d_max, int32_t* d_sum, void* d_tmp, int64_t* d_rets, void* hip_stream);" in hdr
    assert (lib.ROLL_MIN, lib.ROLL_MAX, lib.ROLL_SUM) == (rm.MIN, rm.MAX, rm.SUM) == (1, 2, 4)
    for name, v in (("SPRINTZ_ROLL_MIN", "1u"), ("SPRINTZ_ROLL_MAX", "2u"), ("SPRINTZ_ROLL_SUM", "4u")):
        assert f"#define {name}" in hdr and hdr.split(f"#define {name}")[1].split()[0] == v
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    geom = open(os.path.join(os.path.dirname(HERE), "sprintz_amd", "csrc", "geom.h")).read()
    assert f"kQueryRolling = {Q_ROLLING};" in geom
    from sprintz_amd import ChunkedCodec
    assert callable(ChunkedCodec.rolling_rows)


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=8 * 640, D=8, W=64, ops=7, flags=0, mn=p + 2048, mx=p + 4096, sm=p + 6144, tmp=p + 8192, rets=p + 12288)

    def call(**kw):
        a = dict(good, **kw)
        return lib.rolling_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["W"], a["ops"], a["flags"],
                                a["mn"], a["mx"], a["sm"], a["tmp"], a["rets"], None)

    def refused(code, **kw):
        assert call(**kw) == code, kw
        assert "rolling_rows" in lib.last_error(), (kw, lib.last_error())

    refused(E.E_INVALID, cl=8 * 640 + 1)                                         # chunk_len % ndims != 0
    refused(E.E_INVALID, D=7)
    refused(E.E_INVALID, cl=0)
    refused(E.E_INVALID, flags=2)                                                # unknown flag
    for W in (0, 4, 12, 63, 65):                                                 # below 8, not a multiple of 8
        refused(E.E_INVALID, W=W)
    refused(E.E_INVALID, W=648)                                                  # above R = 640
    refused(E.E_INVALID, W=640 + 8, cl=8 * 647)                                  # above R = 647, which is no multiple of 8
    for ops in (0, 8, 15):
        refused(E.E_INVALID, ops=ops)
    for k, bit in (("mn", 1), ("mx", 2), ("sm", 4)):
        refused(E.E_INVALID, **{k: None})                                        # an op without its output
        refused(E.E_INVALID, ops=7 & ~bit)                                       # an output without its op
    refused(E.E_INVALID, mn=p + 2049)                                            # misaligned outputs
    refused(E.E_INVALID, mx=p + 4097)
    refused(E.E_INVALID, sm=p + 6146)
    refused(E.E_INVALID, rets=p + 12292)
    refused(E.E_INVALID, tmp=None)                                               # more than one chunk: the seam scratch
    refused(E.E_INVALID, tmp=p + 8200)
    for k in ("comp", "offs"):
        refused(E.E_INVALID, **{k: None})
    assert call(D=0) == E.E_INVALID and call(codec=9) == E.E_INVALID and call(esz=3) == E.E_INVALID
    refused(E.E_UNSUPPORTED, D=513, cl=513 * 64)                                 # more than 512 columns
    for codec in (2, 3):
        refused(E.E_UNSUPPORTED, codec=codec)                                    # the non-RLE codecs
    # the sum's int32: 8-bit elements take W up to 8 421 504 by that rule, 16-bit ones up to 32 768 (32 768 x 65 535 = 2^31 - 32 768) -- both far above the LDS bound, which
    # refuses first wherever R allows such a window; the rule itself shows where the shape's LDS bound is beyond it: never, so it is
    # asserted on the formula
    assert rm.sum_max_window(1) * 255 < 1 << 31 <= (rm.sum_max_window(1) + 8) * 255
    assert rm.sum_max_window(2) * 65535 < 1 << 31 <= (rm.sum_max_window(2) + 8) * 65535
    # the LDS bound: the largest W is named
    wmax = rm.max_window(2, 8, False)
    assert wmax == 312
    refused(E.E_UNSUPPORTED, W=wmax + 8, cl=8 * 1024)
    assert f"largest window_rows allowed is {wmax}" in lib.last_error()
    assert call(n=0) == 0                                                        # nothing to do: returns 0, launches nothing
    import torch
    if not torch.cuda.is_available():
        assert call() == E.E_NO_DEVICE
        assert call(W=wmax, cl=8 * 1024) == E.E_NO_DEVICE                        # the largest window passes every check
        assert call(n=1, tmp=None, rets=None) == E.E_NO_DEVICE                   # one chunk needs no scratch
        for ops in rm.SUBSETS:
            outs = {k: (good[k] if ops & bit else None) for k, bit in (("mn", 1), ("mx", 2), ("sm", 4))}
            assert call(ops=ops, **outs) == E.E_NO_DEVICE, ops
        assert call(flags=1) == E.E_NO_DEVICE and call(mn=p + 2050, sm=p + 6148) == E.E_NO_DEVICE


# ------------------------------------------------------------------ the model

def adversarial(name, G, D, W, esz, rng):
    top = (1 << (8 * esz)) - 1
    r = np.arange(G, dtype=np.int64)[:, None] + np.arange(D, dtype=np.int64)[None, :] * 3
    if name == "zeros":
        m = np.zeros((G, D), np.int64)
    elif name == "ones":
        m = np.full((G, D), top, np.int64)
    elif name == "saw-":
        m = r % (W - 1) * (top // W)
    elif name == "saw+":
        m = r % (W + 1) * (top // (W + 1))
    elif name == "falling":
        m = top - r
    elif name == "rising":
        m = r
    else:
        m = rng.integers(0, top + 1, (G, D))
    assert m.min() >= 0 and m.max() <= top
    return m.astype(DTYPES[esz]).reshape(-1)


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("name", ["random", "zeros", "ones", "saw-", "saw+", "falling", "rising"])
def test_model_equals_brute_force(esz, name):
    rng = np.random.default_rng(esz)
    for D, G, W, cut in ((1, 61, 8, 0), (3, 50, 16, 1), (8, 40, 24, 5), (5, 150, 64, 0)):
        x = adversarial(name, G, D, W, esz, rng)[:G * D - cut]            # cut: a partial last row
        got, want = rm.rolling(x, D, W), rm.brute(x, D, W)
        for k in ("min", "max", "sum"):
            assert got[k].dtype == want[k].dtype and got[k].size == x.size and np.array_equal(got[k], want[k]), (name, D, W, k)
        if name == "falling":                                              # the minimum is the newest row, the maximum the row about to leave
            g, d = np.arange(x.size) // D, np.arange(x.size) % D
            assert np.array_equal(got["min"], x) and np.array_equal(got["max"], x[np.maximum(g - W + 1, 0) * D + d])
        if name == "rising":
            g, d = np.arange(x.size) // D, np.arange(x.size) % D
            assert np.array_equal(got["max"], x) and np.array_equal(got["min"], x[np.maximum(g - W + 1, 0) * D + d])
        if name == "ones":
            assert np.array_equal(got["sum"], (rm.counts(-(-x.size // D), W)[np.arange(x.size) // D] * ((1 << (8 * esz)) - 1)).astype(np.int32))


@pytest.mark.parametrize("esz,D,chunk_len,n", [s for s in RAGGED_SHAPES if s[2] // s[1] >= 8])
def test_chunk_local_model(esz, D, chunk_len, n):
    """with every chunk its own beginning the results differ from the true ones only in the first W - 1 rows of the chunks behind the first"""
    rng = np.random.default_rng(n)
    x = rng.integers(0, 1 << (8 * esz), n).astype(DTYPES[esz])
    W = 8
    true, local = rm.rolling(x, D, W), rm.rolling_local(x, chunk_len, D, W)
    e = np.arange(n)
    seam = (e >= chunk_len) & (e % chunk_len // D < W - 1)
    for k in ("min", "max", "sum"):
        assert np.array_equal(true[k][~seam], local[k][~seam])
    assert np.all(true["sum"][seam] >= local["sum"][seam]) and np.any(true["sum"][seam] > local["sum"][seam])


# ------------------------------------------------------------------ rowops

def test_rowops_helpers():
    import torch
    from sprintz_amd import rowops
    for G, W in ((1, 8), (7, 8), (8, 8), (100, 16), (64, 64)):
        c = rowops.rolling_counts(G, W)
        assert c.dtype == torch.int32 and np.array_equal(c.numpy(), rm.counts(G, W))
    rng = np.random.default_rng(1)
    D, G, W = 5, 90, 24
    x = rng.integers(0, 65536, G * D).astype(np.uint16)
    total = rm.rolling(x, D, W)["sum"]
    got = rowops.rolling_mean(torch.from_numpy(total).view(G, D), rowops.rolling_counts(G, W))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy().reshape(-1).view(np.uint32), rm.mean(total, D, W).view(np.uint32))
    # a sum above 2^24 is rounded once, to float32, before the divide
    big = torch.tensor([[312 * 65535]], dtype=torch.int32)
    assert rowops.rolling_mean(big, torch.tensor([312], dtype=torch.int32)).item() == float(np.float32(312 * 65535) / np.float32(312))
    assert rowops.rolling_window(64, 64, 2) == 64 and rowops.rolling_window(8, 640, 1) == 8
    for W, R, esz in ((0, 64, 2), (4, 64, 2), (12, 64, 2), (72, 64, 2), (8.5, 64, 2), (32776, 40000, 2), (8421512, 9000000, 1)):
        assert not (W == int(W) and rm.check_window(int(W), R, esz))
        with pytest.raises(ValueError):
            rowops.rolling_window(W, R, esz)
    assert rowops.rolling_window(32768, 40000, 2) == 32768 and rm.check_window(32768, 40000, 2) and rm.sum_max_window(2) == 32768
    assert rowops.rolling_tmp_bytes(1, 64, 8, 2) == 0
    for n, W, D, esz in ((2, 8, 1, 1), (5, 64, 8, 2), (7, 16, 3, 1), (3, 312, 8, 2)):
        assert rowops.rolling_tmp_bytes(n, W, D, esz) == n * rm.tmp_stride(W, D, esz) and rm.tmp_stride(W, D, esz) % 16 == 0
        assert rm.tmp_stride(W, D, esz) >= 16 + (W - 1) * D * esz
    assert rowops.ROLLING_OPS == ("min", "max", "sum", "mean")


# ------------------------------------------------------------------ the planner

@pytest.fixture(scope="module")
def plan():
    planner.available()
    return lambda **fields: planner.ask("decode", q=Q_ROLLING, **fields)


def named_chunk_len(D):
    return D * (16 * 4 + 3)


@pytest.mark.parametrize("esz,D", FAST_SHAPES + GENERIC_SHAPES)
def test_planner_family_and_lds(plan, esz, D):
    """the family for every named shape, from the planner's rules restated in rolling_model: decode_fast.h for rows of whole 16-byte pieces on
    a one-column-a-lane mapping (8 .. 64 columns) with the chunk's ring behind the groups' carves at table_off, the generic kernel -- the rings
    alone as its LDS -- for everything else and under NO_FAST; misaligned outputs go to the generic kernel"""
    chunk_len = named_chunk_len(D)
    seen = set()
    for general in (0, 1):
        dp = rm.lanes(esz, D, general)
        fdp, _, carve = rm.fast_map(esz, D)
        for W in (8, 16, 64):
            for ops_esz in (esz, 4):                                             # without and with the sum
                for no_fast in (0, 1):
                    for cpg in (1, 3):
                        for out_lo in (0, 4):
                            got = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=7, codec=1, rows=W, out_esz=ops_esz, general=general, no_fast=no_fast,
                                       chunks_per_group=cpg, out_lo=out_lo)
                            ring = rm.ring_bytes(W, D, esz)
                            if rm.fast_takes(esz, D, chunk_len, W, general, no_fast, out_lo, ops_esz):
                                groups = rm.THREADS // fdp
                                assert got.get("family") == "dec_fast", got
                                assert got["lds_group_stride"] == carve and got["table_off"] == carve * groups and got["lds"] == (carve + ring) * groups, got
                                assert got["dp"] == fdp and got["cpl"] == 1 and got["chunks_per_group"] == cpg and got["grid"] == -(--(-7 // cpg) * fdp // rm.THREADS), got
                            else:
                                assert got.get("family") == "dec_generic", got
                                assert got["lds_group_stride"] == ring and got["lds"] == ring * (rm.THREADS // dp) and got["table_off"] == 0, got
                                assert got["log2DP"] == dp.bit_length() - 1 and got["grid"] == -(-7 * dp // rm.THREADS) and got["vec_store"] == 0, got
                            seen.add(got["family"])
    assert seen == ({"dec_fast", "dec_generic"} if (esz, D) in ((2, 8), (2, 16), (2, 24), (2, 64), (1, 16)) else {"dec_generic"})


@pytest.mark.parametrize("esz,D", [(2, 8), (2, 16), (2, 24), (2, 32), (1, 16), (1, 32), (1, 64)])
def test_planner_hands_over_at_the_fast_lds_budget(plan, esz, D):
    """both sides of the edge (f.ring + roll_ring) x groups <= kHistFastLdsBudget, computed from geom.h's formulas restated: the largest such W
    runs decode_fast.h, the next one the generic kernel"""
    dp, cpl, carve = rm.fast_map(esz, D)
    groups = rm.THREADS // dp
    w = rm.fast_max_window(esz, D)
    assert cpl == 1 and w >= 8 and (carve + rm.ring_bytes(w, D, esz)) * groups <= rm.FAST_LDS_BUDGET < (carve + rm.ring_bytes(w + 8, D, esz)) * groups
    assert w + 8 <= rm.max_window(esz, D, False)                                 # (the generic kernel still takes the next one)
    chunk_len = D * (w + 24)
    inside = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=5, codec=0, rows=w, out_esz=4)
    assert inside.get("family") == "dec_fast" and inside["lds"] == (carve + rm.ring_bytes(w, D, esz)) * groups and inside["table_off"] == carve * groups, inside
    beyond = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=5, codec=0, rows=w + 8, out_esz=4)
    assert beyond.get("family") == "dec_generic" and beyond["lds"] == rm.ring_bytes(w + 8, D, esz) * (rm.THREADS // rm.lanes(esz, D, False)), beyond
    if (esz, D) == (2, 8):                                                       # the headline shape: f.ring 1 216 bytes, 32 groups; W = 64 is inside
        assert carve == 1216 and groups == 32 and w >= 64


@pytest.mark.parametrize("esz,D", FAST_SHAPES + GENERIC_SHAPES + [(2, 512), (1, 300)])
def test_planner_refuses_beyond_the_lds_bound(plan, esz, D):
    """both sides of the edge where the rings of a workgroup's chunks stop fitting its 160 KB: the largest window is taken, the next is not"""
    for general in (0, 1):
        wmax = rm.max_window(esz, D, general)
        groups = rm.THREADS // rm.lanes(esz, D, general)
        assert wmax >= 8 and wmax % 8 == 0
        assert rm.ring_bytes(wmax, D, esz) * groups <= rm.LDS_MAX < rm.ring_bytes(wmax + 8, D, esz) * groups
        chunk_len = D * (wmax + 16)
        inside = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=3, codec=0, rows=wmax, out_esz=4, general=general)
        assert inside.get("family") == "dec_generic" and inside["lds"] == rm.ring_bytes(wmax, D, esz) * groups <= rm.LDS_MAX, inside
        beyond = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=3, codec=0, rows=wmax + 8, out_esz=4, general=general)
        assert beyond.get("error") == -4 and "rolling_rows" in beyond["what"], beyond              # SPRINTZ_E_UNSUPPORTED
    for bad in (0, 4, 12):                                                       # never a window the kernels' block structure cannot take
        assert "error" in plan(esz=esz, D=D, chunk_len=D * 640, nchunks=3, codec=0, rows=bad, out_esz=esz)


def test_planner_leaves_the_other_modes_alone(plan):
    """rows and out_esz mean nothing to the plain decode: its plan is the one it had"""
    base = dict(esz=2, D=8, chunk_len=5120, nchunks=4096, codec=1)
    assert planner.ask("decode", **base) == planner.ask("decode", rows=64, **base)
    assert planner.ask("decode", **base)["family"] == "dec_fast"
