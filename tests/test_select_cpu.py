"""CPU tests of select rows (sprintz_mi355x_select_rows): the symbol and its binding are there, every validation return comes before
the device is touched, the numpy model the GPU tier compares with (tests/select_model.py) equals a one-row-at-a-time brute force and
agrees with the filter model's row numbers, and the planner (sprintz_amd/csrc/plan.h, built with g++: tests/plan_probe.cpp)
sends the mode to decode_fast.h or to the generic kernel where the header says."""
import os

import numpy as np
import pytest

import filter_model as fm
import select_model as sm
from fixtures import buf_fixture, lib, random_mask  # noqa: F401  (fixtures)
from planner import QUERY, family, plan_fixture
from rowdata import RAGGED_SHAPES as SHAPES

HERE = os.path.dirname(os.path.abspath(__file__))


buf = buf_fixture(8192)


def test_symbol_and_binding(lib):
    assert "sprintz_mi355x_select_rows" in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.lib, "sprintz_mi355x_select_rows")
    assert len(lib.select_rows.argtypes) == 15
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_select_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    from sprintz_amd import ChunkedCodec
    assert callable(ChunkedCodec.select_rows) and callable(ChunkedCodec.where)


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=5120, D=8, mask=p + 128, bases=p + 1024, cap=100, flags=0, out=p + 2048,
                ids=p + 4096, rets=p + 6144)

    def call(**kw):
        a = dict(good, **kw)
        return lib.select_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["mask"], a["bases"], a["cap"],
                               a["flags"], a["out"], a["ids"], a["rets"], None)

    assert call(cl=5121) == E.E_INVALID and call(cl=5120, D=7) == E.E_INVALID   # chunk_len % ndims != 0
    assert "select_rows" in lib.last_error()
    assert call(cl=0) == E.E_INVALID and call(cl=(1 << 30) + 8) == E.E_INVALID   # chunk_len outside 1..2^30
    assert call(flags=2) == E.E_INVALID and call(flags=3) == E.E_INVALID         # unknown flag (GENERAL_LAYOUT = 1 is the only one)
    for k in ("comp", "offs", "mask", "bases", "out"):
        assert call(**{k: None}) == E.E_INVALID, k                               # NULL pointers
    assert call(out=p + 2049) == E.E_INVALID                                     # d_out not aligned to the element size
    assert call(bases=p + 1028) == E.E_INVALID                                   # d_bases, d_ids, d_rets not aligned to 8 bytes
    assert call(ids=p + 4100) == E.E_INVALID
    assert call(rets=p + 6148) == E.E_INVALID
    assert call(D=0) == E.E_INVALID and call(codec=9) == E.E_INVALID and call(esz=3) == E.E_INVALID
    assert call(D=513, cl=513 * 16) == E.E_UNSUPPORTED                           # more than 512 columns
    for codec in (2, 3):
        assert call(codec=codec) == E.E_UNSUPPORTED                              # the non-RLE codecs
    assert call(codec=4, esz=1) == E.E_UNSUPPORTED
    assert "select_rows" in lib.last_error()
    assert call(n=0) == 0                                                        # nothing to do: returns 0, launches nothing
    import torch
    if not torch.cuda.is_available():
        assert call() == E.E_NO_DEVICE
        assert call(ids=None) == E.E_NO_DEVICE and call(rets=None) == E.E_NO_DEVICE and call(ids=None, rets=None) == E.E_NO_DEVICE
        assert call(esz=1, out=p + 2049, mask=p + 129) == E.E_NO_DEVICE          # 8-bit rows and the mask may lie anywhere
        assert call(out=p + 2050) == E.E_NO_DEVICE                               # an output off the 16-byte grid is the generic kernel's
        assert call(flags=1, D=512, cl=512 * 16) == E.E_NO_DEVICE
        assert call(cap=0) == E.E_NO_DEVICE and call(cap=(1 << 64) - 1) == E.E_NO_DEVICE


@pytest.mark.parametrize("esz,D,chunk_len,n", SHAPES)
def test_model_equals_brute_force(esz, D, chunk_len, n):
    rng = np.random.default_rng(n + D)
    x = rng.integers(0, 1 << (8 * esz), n).astype(np.uint8 if esz == 1 else np.uint16)
    R, MB = fm.geometry(chunk_len, D)
    nchunks = -(-n // chunk_len)
    for p in (0.0, 0.03, 0.5, 1.0):
        mask = random_mask(rng, nchunks, MB, p)              # bits of rows that do not exist are set too: they are ignored
        cnt = sm.counts(mask, n, chunk_len, D)
        total = int(cnt.sum())
        layouts = [sm.prefix_bases(cnt), sm.prefix_bases(cnt[::-1])[::-1], sm.prefix_bases(cnt + 5)]
        for bases in layouts:
            rows_out = int((bases + cnt).max()) + 3
            for cap in (rows_out, total // 2, 0):
                got = sm.select_rows(x, chunk_len, D, mask, bases, cap, out_rows=rows_out, sentinel=7, id_sentinel=-9)
                want = sm.select_rows_brute(x, chunk_len, D, mask, bases, cap, out_rows=rows_out, sentinel=7, id_sentinel=-9)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (p, cap)
        if p == 1.0:                                         # every bit set: the rows that exist, in order
            rows, ids = sm.select_rows(x, chunk_len, D, mask, layouts[0], total)
            exist = np.concatenate([c * R + np.arange(ne // D) for c, ne in enumerate(fm.chunk_counts(n, chunk_len))])
            assert np.array_equal(ids, exist)
            full = np.concatenate([x[c * chunk_len:c * chunk_len + ne // D * D] for c, ne in enumerate(fm.chunk_counts(n, chunk_len))])
            assert np.array_equal(rows.ravel(), full)
        if p == 0.0:
            assert total == 0


@pytest.mark.parametrize("esz,D,chunk_len,n", [s for s in SHAPES if s[3] % s[1] == 0])
def test_model_with_the_filter_models_mask(esz, D, chunk_len, n):
    rng = np.random.default_rng(n)
    top = (1 << (8 * esz)) - 1
    x = rng.integers(0, top + 1, n).astype(np.uint8 if esz == 1 else np.uint16)
    lo, hi = np.zeros(D, np.int64), np.full(D, top, np.int64)
    lo[0], hi[D - 1] = top // 4, 3 * top // 4
    for mode in (fm.ALL, fm.ANY):
        mask, cnt = fm.filter_rows(x, chunk_len, D, lo if mode == fm.ALL else hi, hi if mode == fm.ALL else lo + top // 2, mode)
        assert np.array_equal(cnt, sm.counts(mask, n, chunk_len, D))
        want_ids = fm.row_ids(mask, chunk_len, D)
        rows, ids = sm.select_rows(x, chunk_len, D, mask, sm.prefix_bases(cnt), int(cnt.sum()))
        assert np.array_equal(ids, want_ids)
        assert np.array_equal(rows, x.reshape(-1, D)[want_ids])


plan = plan_fixture(shape=family, q=QUERY["select"], codec=1, nchunks=4096, capacity=1000, out_lo=0)


def test_planner_edges(plan):
    fast = [(1, 16, 16 * 512), (2, 8, 5120), (1, 80, 10240), (2, 24, 24 * 200)]
    for esz, D, cl in fast:
        for codec in (0, 1):
            assert plan(esz=esz, D=D, chunk_len=cl, codec=codec) == "dec_fast", (esz, D, cl)
        assert plan(esz=esz, D=D, chunk_len=cl, no_fast=1) == "dec_generic", (esz, D, cl)
        for out_lo in (1, 2, 8, 15):
            assert plan(esz=esz, D=D, chunk_len=cl, out_lo=out_lo) == "dec_generic", (esz, D, cl, out_lo)
        # capacity * D * esz on either side of 0xf0000000, in 64 bits
        edge = (0xf0000000 - 1) // (D * esz)
        assert (edge * D * esz < 0xf0000000) and ((edge + 1) * D * esz >= 0xf0000000)
        assert plan(esz=esz, D=D, chunk_len=cl, capacity=edge) == "dec_fast", (esz, D, cl)
        assert plan(esz=esz, D=D, chunk_len=cl, capacity=edge + 1) == "dec_generic", (esz, D, cl)
        assert plan(esz=esz, D=D, chunk_len=cl, capacity=(1 << 64) - 1) == "dec_generic"      # (no wrap of the product)
        assert plan(esz=esz, D=D, chunk_len=cl, capacity=(1 << 32) // (D * esz) * (1 << 32) + 1) == "dec_generic"
        assert plan(esz=esz, D=D, chunk_len=cl, capacity=0) == "dec_fast"
    generic = [(2, 12, 12 * 400),                                  # rows that are not whole 16-byte pieces
               (1, 1, 1024), (2, 1, 1024), (1, 2, 2048), (2, 2, 2048), (1, 3, 3000),   # the low-dimension layouts: decode_uni.h is not taught
               (2, 300, 9600), (1, 300, 9600),                     # more than 256 columns
               (1, 8, 4096), (2, 4, 4096), (1, 24, 24 * 200)]      # general layout, rows of 8 / 8 / 24 bytes
    for esz, D, cl in generic:
        for general in (0, 1):
            assert plan(esz=esz, D=D, chunk_len=cl, general=general) == "dec_generic", (esz, D, cl, general)
    # the mode never reaches the small-batch and block-parallel kernels, whatever the batch size
    for nchunks in (1, 64, 2048, 2049, 131072):
        assert plan(esz=2, D=8, chunk_len=5120, nchunks=nchunks) == "dec_fast"
        assert plan(esz=1, D=80, chunk_len=10240, nchunks=nchunks, codec=0) == "dec_fast"
        assert plan(esz=1, D=1, chunk_len=1024, nchunks=nchunks, codec=0) == "dec_generic"
    # the filter's plan is what it was: decode_uni.h still serves it
    assert plan(esz=1, D=1, chunk_len=1024, q=5) == "dec_uni" and plan(esz=2, D=8, chunk_len=5120, q=5, out_lo=3) == "dec_fast"
