"""CPU tests of linear filter rows (sprintz_mi355x_filter_linear): the two symbols and their bindings are there, every validation return
comes before the device is touched, the scratch size behaves, the numpy model the GPU tier compares with (tests/linear_model.py) equals
brute force, rowops.linear_terms takes every form of its arguments and holds the exactness bound, and the planner
(sprintz_amd/csrc/plan.h, built with g++: tests/plan_probe.cpp) sends the mode to decode_fast.h or to the generic kernel, never
to decode_uni.h."""
import ctypes as C
import os

import numpy as np
import pytest

import filter_model as fm
import linear_model as lm
from fixtures import buf_fixture, lib, refusals  # noqa: F401  (fixtures)
from planner import QUERY, plan_fixture, split

HERE = os.path.dirname(os.path.abspath(__file__))
Q_LINEAR = QUERY["linear"]


buf = buf_fixture(65536)


def test_symbols_and_bindings(lib):
    for s in ("sprintz_mi355x_filter_linear", "sprintz_mi355x_filter_linear_tmp_bytes"):
        assert s in lib.EXPORTED_SYMBOLS and hasattr(lib.lib, s)
    assert len(lib.filter_linear.argtypes) == 18 and len(lib.filter_linear_tmp_bytes.argtypes) == 3
    assert lib.filter_linear_tmp_bytes.restype is C.c_uint64
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_filter_linear(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    assert "uint32_t chunk_len, uint16_t ndims, const int32_t* d_weights, const int32_t* d_lag_weights," in hdr
    assert "int32_t bias, int32_t lo, int32_t hi, uint32_t flags, void* d_tmp, uint8_t* d_mask, uint32_t* d_counts," in hdr
    assert "uint64_t sprintz_mi355x_filter_linear_tmp_bytes(int elem_bytes, uint64_t nchunks, uint16_t ndims);" in hdr
    assert "< 2^31" in hdr and "wrapping 32-bit" in hdr             # the wrapping rule and the exactness bound are the header's to state
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33            # additive: no new ABI version, no new kernel family
    geom = open(os.path.join(os.path.dirname(HERE), "sprintz_amd", "csrc", "geom.h")).read()
    assert f"kQueryLinear = {Q_LINEAR}" in geom
    from sprintz_amd import ChunkedCodec
    assert callable(ChunkedCodec.filter_linear) and callable(ChunkedCodec.filter_change)


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=5120, D=8, w=p + 128, u=p + 256, bias=0, lo=-5, hi=5, flags=0, tmp=p + 1024,
                mask=p + 4096, counts=p + 8192, rets=p + 16384)

    def call(**kw):
        a = dict(good, **kw)
        return lib.filter_linear(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["w"], a["u"], a["bias"], a["lo"], a["hi"],
                                 a["flags"], a["tmp"], a["mask"], a["counts"], a["rets"], None)

    invalid, unsupported = refusals(lib, call)

    invalid(flags=2)                                                             # unknown flag (GENERAL_LAYOUT = 1 is the only one)
    invalid(flags=3)
    for k in ("comp", "offs", "w"):                                              # NULL d_comp / d_offsets / d_weights
        invalid(**{k: None})
    invalid(mask=None, counts=None)                                              # neither a mask nor counts
    assert "filter_linear" in lib.last_error()
    invalid(cl=5121)                                                             # chunk_len % ndims != 0
    assert "filter_linear" in lib.last_error()
    invalid(D=7)
    invalid(cl=0)
    invalid(cl=(1 << 30) + 8)
    for off in (1, 2, 3):
        invalid(w=good["w"] + off)                                               # weights not aligned to 4 bytes
        invalid(u=good["u"] + off)
        invalid(counts=good["counts"] + off)                                     # counts not aligned to 4 bytes
    for off in (1, 2, 4):
        invalid(rets=good["rets"] + off)                                         # rets not aligned to 8 bytes
    invalid(tmp=None)                                                            # lag weights without their scratch
    for off in (1, 2, 4):
        invalid(tmp=good["tmp"] + off)                                           # ... or with scratch that is not 8-aligned
    assert call(D=0) == E.E_INVALID and call(codec=9) == E.E_INVALID and call(esz=3) == E.E_INVALID
    unsupported(D=513, cl=513 * 16)                                              # more than 512 columns
    for codec in (2, 3):
        unsupported(codec=codec)                                                 # the non-RLE codecs
    unsupported(codec=4, esz=1)
    assert call(n=0) == 0                                                        # nothing to do: returns 0, launches nothing
    assert call(n=0, u=None, tmp=None, rets=None) == 0
    import torch
    if not torch.cuda.is_available():
        assert call() == E.E_NO_DEVICE
        assert call(u=None, tmp=None) == E.E_NO_DEVICE                           # no lag term: the scratch is not asked for
        assert call(u=None, tmp=good["tmp"] + 1) == E.E_NO_DEVICE                # ... and may lie anywhere
        assert call(mask=None) == E.E_NO_DEVICE and call(counts=None) == E.E_NO_DEVICE and call(rets=None) == E.E_NO_DEVICE
        assert call(mask=good["mask"] + 1) == E.E_NO_DEVICE                      # the mask may lie anywhere
        assert call(lo=5, hi=-5) == E.E_NO_DEVICE                                # lo > hi is a predicate: nothing matches
        assert call(lo=-(1 << 31), hi=(1 << 31) - 1, bias=-(1 << 31)) == E.E_NO_DEVICE
        assert call(esz=1, codec=0) == E.E_NO_DEVICE and call(flags=1) == E.E_NO_DEVICE
        assert call(D=512, cl=512 * 16) == E.E_NO_DEVICE and call(cl=1 << 30) == E.E_NO_DEVICE


def test_tmp_bytes(lib):
    t = lib.filter_linear_tmp_bytes
    for esz in (1, 2):
        for D in (1, 3, 8, 80, 300, 512):
            for n in (1, 2, 1000, 1 << 20):
                b = t(esz, n, D)
                assert b > 0 and b % 8 == 0
                assert b >= n * (2 * D * esz + 4)            # two rows and a flag a chunk, at least
                assert t(esz, n + 1, D) >= b and (D == 512 or t(esz, n, D + 1) >= b)     # monotone in nchunks and ndims
        assert t(esz, 1, 8) * 1000 == t(esz, 1000, 8)
        assert t(esz, 0, 8) == 0 and t(esz, 5, 0) == 0 and t(esz, 5, 513) == 0
    assert t(0, 5, 8) == 0 and t(3, 5, 8) == 0 and t(-1, 5, 8) == 0
    assert t(2, 1 << 62, 512) == 0                           # a size that does not fit


SHAPES = [
    # test_filter_cpu.py's ragged shapes with whole rows a chunk: (esz, D, chunk_len, n) -- short last chunks, one ending mid-row, R % 8 != 0
    (1, 3, 99, 99 * 4 + 41),
    (2, 5, 80, 80 * 3 + 17),
    (1, 1, 13, 13 * 5 + 6),
    (2, 8, 8 * 21, 8 * 21 * 3 + 8 * 5 + 3),
    (1, 7, 7 * 16, 7 * 16 * 2 + 7 * 9 + 6),
    (2, 2, 64, 64 * 4),
]


@pytest.mark.parametrize("esz,D,chunk_len,n", SHAPES)
def test_model_equals_brute_force(esz, D, chunk_len, n):
    rng = np.random.default_rng(n * 31 + D)
    top = (1 << (8 * esz)) - 1
    x = rng.integers(0, top + 1, n)
    x[rng.integers(0, n, n // 8)] = 0
    x[rng.integers(0, n, n // 8)] = top
    nchunks = -(-n // chunk_len)
    R, MB = fm.geometry(chunk_len, D)
    for trial in range(8):
        big = trial >= 6                                     # the last two wrap: any int32 weights
        wmax = (1 << 31) - 1 if big else ((1 << 31) - 1) // (top * 2 * D) - 1
        w = rng.integers(-wmax, wmax + 1, D)
        u = None if trial % 2 == 0 else rng.integers(-wmax, wmax + 1, D)
        bias = int(rng.integers(-1000, 1000))
        assert big or lm.bound_B(esz, w, u, bias) < 1 << 31
        s = lm.sums(x, D, w, u, bias)
        lo, hi = (None, None) if trial == 0 else sorted(int(v) for v in rng.choice(s, 2)) if trial < 5 else (5, -5) if trial == 5 else (int(s.min()), int(np.median(s)))
        mask, counts = lm.filter_linear(x, chunk_len, D, w, lo, hi, u, bias)
        bm, bc = lm.filter_linear_brute(x, chunk_len, D, w, lo, hi, u, bias)
        assert mask.shape == (nchunks, MB) and mask.dtype == np.uint8
        assert np.array_equal(mask, bm) and np.array_equal(counts, bc), trial
        assert np.array_equal(counts, np.unpackbits(mask, axis=1).sum(axis=1))
        rows = n // D
        assert counts.sum() == (rows if trial == 0 else 0 if trial == 5 else counts.sum())
        if trial == 0:                                       # the open interval: exactly the rows that exist, 0 for the others
            want = np.zeros((nchunks, MB * 8), np.uint8)
            for c in range(nchunks):
                want[c, :max(0, min(R, rows - c * R))] = 1
            assert np.array_equal(np.unpackbits(mask, axis=1, bitorder="little"), want)


def test_model_lag_is_numpy_diff():
    """row 0 is its own predecessor: numpy.diff(..., prepend=x[0]); a chunk's first row looks into the chunk in front"""
    rng = np.random.default_rng(5)
    D, chunk_len = 3, 3 * 10
    x = rng.integers(0, 256, chunk_len * 4 + 3 * 4 + 1)
    v = x[:x.size // D * D].reshape(-1, D)
    d = np.diff(v[:, 1], prepend=v[0, 1])
    mask, counts = lm.filter_change(x, chunk_len, D, 1, lo=10)
    bits = np.unpackbits(mask, axis=1, bitorder="little")[:, :10].reshape(-1)[:v.shape[0]]
    assert np.array_equal(bits, (d >= 10).astype(np.uint8)) and counts.sum() == (d >= 10).sum()
    own, _ = lm.filter_change(x, chunk_len, D, 1, lo=10, self_rows=range(0, v.shape[0], 10))
    assert not (own[:, 0] & 1).any()                         # a row that is its own predecessor changes by 0


def test_linear_terms():
    import torch
    from sprintz_amd import rowops
    dev = torch.device("cpu")
    w, u, bias, lo, hi = rowops.linear_terms({0: 1, 2: -1}, None, 0, 1, None, 4, 2, dev)
    assert w.dtype == torch.int32 and w.tolist() == [1, 0, -1, 0] and u is None and (bias, lo, hi) == (0, 1, (1 << 31) - 1)
    w, u, bias, lo, hi = rowops.linear_terms(1, {3: -2}, -7, None, 9, 4, 1, dev)
    assert w.tolist() == [1, 1, 1, 1] and u.dtype == torch.int32 and u.tolist() == [0, 0, 0, -2] and (bias, lo, hi) == (-7, -(1 << 31), 9)
    w, u, *_ = rowops.linear_terms(torch.tensor([3, -4], dtype=torch.int64), [5, 6], 0, None, None, 2, 1, dev)
    assert w.dtype == torch.int32 and w.tolist() == [3, -4] and u.tolist() == [5, 6] and w.is_contiguous()
    w, *_ = rowops.linear_terms(np.int32(2), None, 0, 0, 0, 3, 2, dev)
    assert w.tolist() == [2, 2, 2]
    for esz in (1, 2):
        top = (1 << (8 * esz)) - 1
        q, r = divmod((1 << 31) - 1, top)                    # B = r + top q = 2^31 - 1 exactly: taken, in every split over w, u and bias
        assert lm.bound_B(esz, [q, 0], None, r) == (1 << 31) - 1
        rowops.linear_terms([q, 0], None, r, None, None, 2, esz, dev)
        rowops.linear_terms([-q, 0], None, -r, None, None, 2, esz, dev)
        rowops.linear_terms([q - 5, 2], [-2, 1], r, None, None, 2, esz, dev)
        for args in (([q, 0], None, r + 1), ([q, 0], None, -r - 1), ([q - 5, 2], [-1, -2], r + 1), ([q - 5, 2], [2, 2], r), ([q + 1, 0], None, 0)):
            assert lm.bound_B(esz, *args) >= 1 << 31         # B = 2^31 (or more): refused
            with pytest.raises(ValueError, match="2\\^31"):
                rowops.linear_terms(args[0], args[1], args[2], None, None, 2, esz, dev)
        assert lm.bound_B(esz, [q, 0], None, r + 1) == 1 << 31
    for lo, hi in (((1 << 31), None), (None, -(1 << 31) - 1), (-(1 << 32), 0)):
        with pytest.raises(ValueError, match="int32"):
            rowops.linear_terms(1, None, 0, lo, hi, 2, 1, dev)
    with pytest.raises(ValueError):
        rowops.linear_terms([1, 2, 3], None, 0, None, None, 2, 1, dev)           # the wrong number of entries
    with pytest.raises(ValueError):
        rowops.linear_terms({2: 1}, None, 0, None, None, 2, 1, dev)              # a column that is not there
    with pytest.raises(ValueError):
        rowops.linear_terms(torch.tensor([1.0, 2.0]), None, 0, None, None, 2, 1, dev)


plan = plan_fixture(shape=split, codec=1, nchunks=4096, q=Q_LINEAR)


def test_plan(plan):
    for codec in (0, 1):
        assert plan(esz=2, D=8, chunk_len=5120, codec=codec)[0] == "dec_fast"                 # the headline shape
        assert plan(esz=2, D=8, chunk_len=5120, codec=codec, no_fast=1)[0] == "dec_generic"
        for esz, D, cl in ((1, 1, 1024), (2, 1, 1024), (1, 2, 1024), (2, 2, 1024), (1, 3, 3 * 512), (1, 4, 4096)):
            assert plan(esz=esz, D=D, chunk_len=cl, codec=codec)[0] == "dec_generic", (esz, D)   # never dec_uni: it is not taught the mode
        assert plan(esz=2, D=300, chunk_len=9600, codec=codec)[0] == "dec_generic"
        assert plan(esz=1, D=300, chunk_len=9600, codec=codec)[0] == "dec_generic"
    # the filter's own plan on the same shapes: decode_uni where this mode goes to the generic kernel, the same family elsewhere
    assert plan(esz=1, D=1, chunk_len=1024, q=5)[0] == "dec_uni"
    for esz, D, cl in ((2, 8, 5120), (1, 80, 10240), (2, 5, 5 * 104), (2, 300, 9600), (2, 3, 300)):
        assert plan(esz=esz, D=D, chunk_len=cl)[0] == plan(esz=esz, D=D, chunk_len=cl, q=5)[0], (esz, D)
        fam, f = plan(esz=esz, D=D, chunk_len=cl)
        if fam == "dec_fast":
            assert f["lds"] == plan(esz=esz, D=D, chunk_len=cl, q=5)[1]["lds"]    # nothing staged: the filter's carve
