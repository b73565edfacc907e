"""CPU tests of moments rows (sprintz_mi355x_moments_rows): the symbol and its binding are there, every validation return comes before
the device is touched and names the operation, the numpy model the GPU tier compares with (tests/moments_model.py) equals a
one-row-at-a-time brute force in Python ints and the aggregate model's sum and count, its exact rationals are what their definitions
say, and the planner (sprintz_amd/csrc/plan.h, built with g++: tests/plan_probe.cpp) sends the mode where
the windowed query goes -- except that decode_uni.h never gets it."""
import os
from fractions import Fraction

import numpy as np
import pytest

import aggregate_model as am
import filter_model as fm
import moments_model as mm
from fixtures import buf_fixture, lib, random_mask, refusals  # noqa: F401  (fixtures)
from planner import QUERY, family, plan_fixture

HERE = os.path.dirname(os.path.abspath(__file__))
Q_WINDOW, Q_AGGREGATE, Q_MOMENTS = QUERY["window"], QUERY["aggregate"], QUERY["moments"]


buf = buf_fixture(16384)


def test_symbol_and_binding(lib):
    assert "sprintz_mi355x_moments_rows" in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.lib, "sprintz_mi355x_moments_rows")
    assert len(lib.moments_rows.argtypes) == 18
    assert (lib.MOM_COUNT, lib.MOM_SUM, lib.MOM_SUMSQ, lib.MOM_CROSS) == (1, 2, 4, 8)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_moments_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    for name, v in (("COUNT", 1), ("SUM", 2), ("SUMSQ", 4), ("CROSS", 8)):
        assert f"#define SPRINTZ_MOM_{name} {v}u" in hdr
    assert "moments_rows, SPRINTZ_MOM_*" in hdr                   # the version comment's "later, additively" list
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    from sprintz_amd import ChunkedCodec
    assert callable(ChunkedCodec.moments_rows) and callable(ChunkedCodec.moments_where) and callable(ChunkedCodec.corr)


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=5120, D=8, mask=p + 128, W=64, ops=15, ref=3, flags=0, cnt=p + 2048, sm=p + 4096,
                sq=p + 6144, cr=p + 8192, rets=p + 10240)

    def call(**kw):
        a = dict(good, **kw)
        return lib.moments_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["mask"], a["W"], a["ops"], a["ref"],
                                a["flags"], a["cnt"], a["sm"], a["sq"], a["cr"], a["rets"], None)

    invalid, unsupported = refusals(lib, call, "moments_rows")

    invalid(cl=5121)                                                             # chunk_len % ndims != 0
    invalid(D=7)
    invalid(cl=0)                                                                # chunk_len outside 1..2^30
    invalid(cl=(1 << 30) + 8)
    for W in (0, 4, 7, 12, 63, 65):                                              # W not a multiple of 8 that is >= 8
        invalid(W=W)
    for ops in (0, 16, 17, 32, 0xFFFFFFFF):                                      # ops outside 1..15
        invalid(ops=ops)
    for k, bit in (("cnt", 1), ("sm", 2), ("sq", 4), ("cr", 8)):                 # a selected output that is NULL
        invalid(**{k: None})
        invalid(**{k: None, "ops": bit})
    for k in ("comp", "offs"):                                                   # NULL pointers (the mask may be NULL)
        invalid(**{k: None})
    for off in (1, 2, 3):
        invalid(cnt=p + 2048 + off)                                              # d_count not aligned to 4 bytes
    for off in (1, 2, 4):
        invalid(sm=p + 4096 + off)                                               # d_sum / d_sumsq / d_cross / d_rets not aligned to 8 bytes
        invalid(sq=p + 6144 + off)
        invalid(cr=p + 8192 + off)
        invalid(rets=p + 10240 + off)
    for ref in (8, 9, 512, 0xFFFFFFFF):                                          # ref_col >= ndims where CROSS is selected
        invalid(ref=ref)
        invalid(ref=ref, ops=8)
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
        assert call(mask=None) == E.E_NO_DEVICE                                  # no mask: every existing row
        for k, bit in (("cnt", 1), ("sm", 2), ("sq", 4), ("cr", 8)):             # an output that is not selected may be NULL
            assert call(**{k: None, "ops": 15 & ~bit}) == E.E_NO_DEVICE, k
        assert call(sm=None, sq=None, cr=None, ops=1) == E.E_NO_DEVICE           # the count alone
        assert call(sq=p + 6145, cr=p + 8193, ops=3) == E.E_NO_DEVICE            # ... and may lie anywhere
        for ref in (8, 0xFFFFFFFF):                                              # ref_col is ignored where CROSS is not selected
            assert call(ref=ref, ops=7) == E.E_NO_DEVICE
        assert call(ref=7) == E.E_NO_DEVICE and call(ref=0) == E.E_NO_DEVICE
        assert call(rets=None) == E.E_NO_DEVICE
        assert call(mask=p + 129) == E.E_NO_DEVICE                               # the mask may lie anywhere
        assert call(W=648) == E.E_NO_DEVICE and call(W=1 << 20) == E.E_NO_DEVICE # W > R: one window a chunk
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


@pytest.mark.parametrize("esz,D,chunk_len,n", SHAPES)
def test_model_equals_brute_force(esz, D, chunk_len, n):
    rng = np.random.default_rng(n + D)
    top = (1 << (8 * esz)) - 1
    x = rng.integers(top - 40, top + 1, n).astype(np.uint8 if esz == 1 else np.uint16)      # near the top: the largest products
    R, MB = fm.geometry(chunk_len, D)
    nchunks = -(-n // chunk_len)
    for p in (0.0, 0.03, 0.5, 1.0, None):
        mask = None if p is None else random_mask(rng, nchunks, MB, p)   # bits of rows that do not exist are set too: they are ignored
        for W in windows_for(R):
            for ref in {0, D - 1, D // 2}:
                got = mm.moments_rows(x, chunk_len, D, mask, W, ref)
                want = mm.moments_rows_brute(x, chunk_len, D, mask, W, ref)
                for k in ("sum", "sumsq", "cross", "count"):
                    assert got[k].tolist() == want[k], (k, p, W, ref)             # Python ints on both sides
                assert got["sumsq"].dtype == np.uint64 and got["count"].dtype == np.uint32 and got["count"].shape == (nchunks, -(-R // W))
                assert np.array_equal(got["cross"][..., ref], got["sumsq"][..., ref])
                empty = got["count"] == 0
                assert all(np.all(got[k][empty] == 0) for k in ("sum", "sumsq", "cross"))
            if p == 0.0:
                assert empty.all()
            if p is None:
                assert int(got["count"].sum()) == n // D
            else:                                               # sum and count are the aggregate model's
                agg = am.aggregate_rows(x, chunk_len, D, mask, W)
                assert np.array_equal(got["sum"], agg["sum"]) and np.array_equal(got["count"], agg["count"])


def test_global_model_folds_the_chunk_windows():
    rng = np.random.default_rng(3)
    D, R = 4, 24
    chunk_len = D * R
    n = chunk_len * 5 + D * 7
    x = rng.integers(0, 65536, n).astype(np.uint16)
    mask = random_mask(rng, 6, 3, 0.3)
    for m in (mask, None):
        for W in (8, 24, 48, 72):                                # R % W == 0 and W % R == 0
            g = mm.global_windows(x, chunk_len, D, m, W, ref=2)
            sel = am.selected(mm.all_rows(n, chunk_len, D) if m is None else m, n, chunk_len, D).reshape(-1)
            rows = np.pad(x, (0, 6 * chunk_len - n)).reshape(-1, D)
            for w in range(g["count"].size):
                pick = np.flatnonzero(sel[w * W:(w + 1) * W]) + w * W
                v = [[int(t) for t in rows[r]] for r in pick]
                assert g["count"][w] == len(v)
                assert g["sum"][w].tolist() == [sum(r[d] for r in v) for d in range(D)]
                assert g["sumsq"][w].tolist() == [sum(r[d] * r[d] for r in v) for d in range(D)]
                assert g["cross"][w].tolist() == [sum(r[d] * r[2] for r in v) for d in range(D)]


def test_exact_rationals():
    xs, ys = [65535, 65534, 65535, 65534, 65535], [1, 3, 1, 3, 2]
    n = len(xs)
    e = mm.exact_derived(n, sum(xs), sum(v * v for v in xs), sum(a * b for a, b in zip(xs, ys)), sum(ys), sum(v * v for v in ys))
    mx, my = Fraction(sum(xs), n), Fraction(sum(ys), n)
    assert e["mean"] == mx
    assert e["var"] == sum((v - mx) ** 2 for v in xs) / n == Fraction(6, 25)
    assert e["cov"] == sum((a - mx) * (b - my) for a, b in zip(xs, ys)) / n
    assert e["corr2"] == e["cov"] ** 2 / (e["var"] * sum((v - my) ** 2 for v in ys) / n) and e["sign"] == -1
    assert abs(mm.corr_float(e) + float(e["corr2"]) ** 0.5) < 1e-15
    e1 = mm.exact_derived(n, sum(xs), sum(v * v for v in xs), ddof=1)
    assert e1["var"] == sum((v - mx) ** 2 for v in xs) / (n - 1)
    assert mm.exact_derived(0, 0, 0)["mean"] is None and mm.exact_derived(1, 5, 25, ddof=1)["var"] is None
    const = mm.exact_derived(3, 15, 75, 30, 6, 14)              # x constant: no correlation
    assert const["var"] == 0 and const["corr2"] is None and np.isnan(mm.corr_float(const))


plan = plan_fixture(shape=family, codec=1, nchunks=4096, q=Q_MOMENTS)


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
    # across a sweep of shapes: the windowed query's family, with decode_uni.h replaced by the generic kernel
    for esz in (1, 2):
        for D in (1, 2, 3, 4, 5, 8, 12, 16, 33, 64, 80, 128, 200, 256, 300, 512):
            for rows in (13, 64, 200, 1024):
                for general in (0, 1):
                    w = plan(esz=esz, D=D, chunk_len=D * rows, general=general, q=Q_WINDOW)
                    assert plan(esz=esz, D=D, chunk_len=D * rows, general=general) == ("dec_generic" if w == "dec_uni" else w), (esz, D, rows, general)
    # the other modes' plans are what they were
    assert plan(esz=1, D=1, chunk_len=1024, q=5) == "dec_uni" and plan(esz=1, D=1, chunk_len=1024, q=6) == "dec_generic"
    assert plan(esz=1, D=1, chunk_len=1024, q=Q_AGGREGATE) == "dec_generic" and plan(esz=2, D=8, chunk_len=5120, q=Q_AGGREGATE) == "dec_fast"
