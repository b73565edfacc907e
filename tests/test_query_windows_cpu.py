"""CPU tests of the windowed query (sprintz_mi355x_query_windows): argument validation before the device is touched,
and the numpy model of its semantics (tests/window_model.py) against brute-force loops on the edge shapes."""
import ctypes as C
import os

import numpy as np
import pytest

import window_model as wm
from fixtures import lib  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_windows_validation(lib):
    buf = (C.c_uint8 * 4096)()
    p = (C.addressof(buf) + 15) & ~15
    E = lib

    def q(codec=1, esz=2, comp=p, offs=p, n=1, chunk_len=64, D=8, W=8, ops=7, flags=0, mn=p, mx=p + 256, sm=p + 512, rets=None):
        return lib.query_windows(codec, esz, comp, offs, n, chunk_len, D, W, ops, flags, mn, mx, sm, rets, None)

    # check_common
    assert q(codec=9) == E.E_INVALID
    assert q(esz=3) == E.E_INVALID
    assert q(D=0) == E.E_INVALID
    assert q(codec=4, esz=2) == E.E_UNSUPPORTED                                   # xff_norle is 8-bit only
    # window_rows: a multiple of 8, at least 8
    for W in (0, 1, 4, 7, 12, 65):
        assert q(W=W) == E.E_INVALID, W
    # ops in 1..7
    for ops in (0, 8, 15, 0xffffffff):
        assert q(ops=ops) == E.E_INVALID, ops
    # a selected output must not be NULL
    assert q(ops=1, mn=None) == E.E_INVALID
    assert q(ops=2, mx=None) == E.E_INVALID
    assert q(ops=4, sm=None) == E.E_INVALID
    assert q(ops=7, sm=None) == E.E_INVALID
    # alignment: min / max to the element size, sum to 8 bytes
    assert q(mn=p + 1) == E.E_INVALID
    assert q(mx=p + 1) == E.E_INVALID
    assert q(sm=p + 4) == E.E_INVALID
    # unknown flag
    assert q(flags=2) == E.E_INVALID
    assert q(flags=0x80000000) == E.E_INVALID
    # more than 512 columns: refused before the device
    assert q(D=513, chunk_len=513 * 16) == E.E_UNSUPPORTED
    assert q(D=4096, chunk_len=4096 * 16) == E.E_UNSUPPORTED
    # as query_batch: chunk_len and the container
    assert q(chunk_len=0) == E.E_INVALID
    assert q(comp=None) == E.E_INVALID
    assert q(offs=None) == E.E_INVALID

    import torch
    if torch.cuda.is_available():
        return
    # valid arguments reach the device check; outputs that are not selected may be NULL, as may unaligned ones
    assert q() == E.E_NO_DEVICE
    assert q(ops=1, mx=None, sm=None) == E.E_NO_DEVICE
    assert q(ops=2, mn=None, sm=None) == E.E_NO_DEVICE
    assert q(ops=4, mn=p + 1, mx=None) == E.E_NO_DEVICE
    assert q(esz=1, mn=p + 1, mx=p + 3, codec=0) == E.E_NO_DEVICE
    assert q(flags=1, D=512, chunk_len=512 * 16, W=4096) == E.E_NO_DEVICE
    assert q(codec=2, esz=1, n=0) == E.E_NO_DEVICE
    assert "no CPU fallback" in lib.last_error() or lib.last_error()


def test_query_windows_constants_and_binding(lib):
    text = open(os.path.join(ROOT, "include", "sprintz_mi355x.h")).read()
    for name, val in (("MIN", 1), ("MAX", 2), ("SUM", 4)):
        assert f"#define SPRINTZ_QUERY_WIN_{name} {val}u" in text
        assert getattr(lib, f"QUERY_WIN_{name}") == val
    assert "sprintz_mi355x_query_windows" in lib.EXPORTED_SYMBOLS


# (n, chunk_len, ndims, W): the edge shapes of the semantics
EDGE = [
    ("partial last row", 8 * 37 + 5, 64, 8, 8),
    ("chunk_len % ndims != 0", 3 * 100 + 41, 100, 3, 8),
    ("short last chunk", 5 * 640 + 96, 640, 8, 24),
    ("W > R", 4 * 160 + 17, 160, 5, 64),
    ("W = 8 over a verbatim tail", 3 * (16 * 4 * 3 + 4 * 11) + 7, 16 * 4 * 3 + 4 * 11, 4, 8),
    ("one column", 1000, 256, 1, 16),
    ("many columns, no groups", 2 * 1000 + 300, 1000, 200, 8),
]


@pytest.mark.parametrize("name,n,chunk_len,ndims,W", EDGE)
@pytest.mark.parametrize("esz", [1, 2])
def test_model_chunk_windows_match_brute_force(name, n, chunk_len, ndims, W, esz):
    rng = np.random.default_rng(n * 7 + esz)
    x = rng.integers(0, 1 << (8 * esz), n).astype(np.uint8 if esz == 1 else np.uint16)
    got = wm.chunk_windows(x, chunk_len, ndims, W)
    want = wm.brute_chunk_windows(x, chunk_len, ndims, W)
    for g, w, k in zip(got, want, ("min", "max", "sum")):
        assert g.shape == w.shape, (name, k)
        assert np.array_equal(g.astype(np.int64), w.astype(np.int64)), (name, k)
    mn, mx, sm = got
    # identities where a window has no element
    nchunks = mn.shape[0]
    R = -(-chunk_len // ndims)
    for c in range(nchunks):
        nc = min(chunk_len, n - c * chunk_len)
        for w in range(mn.shape[1]):
            for d in range(ndims):
                empty = not any((e // ndims) // W == w and e % ndims == d for e in range(d, nc, ndims))
                if empty:
                    assert mn[c, w, d] == (1 << (8 * esz)) - 1 and mx[c, w, d] == 0 and sm[c, w, d] == 0, (name, c, w, d)
    assert mn.shape[1] == -(-R // W)


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("n,chunk_len,ndims,W", [
    (8 * 64 * 5 + 8 * 3, 8 * 64, 8, 16),      # W divides R; partial last window
    (8 * 64 * 5 + 8 * 3, 8 * 64, 8, 64),      # W = R
    (8 * 64 * 7 + 5, 8 * 64, 8, 192),         # W a multiple of R (the fold); partial last row and window
    (3 * 50 * 9 + 2, 3 * 50, 3, 100),         # R = 50, not a multiple of 8: the kernel takes one window of 56 rows a chunk
    (1024 * 5, 1024, 1, 8),
    (5 * 80 * 128 + 80 * 3, 80 * 128, 80, 32),
])
def test_model_global_windows_and_fold(esz, n, chunk_len, ndims, W):
    rng = np.random.default_rng(n + W)
    x = rng.integers(0, 1 << (8 * esz), n).astype(np.uint8 if esz == 1 else np.uint16)
    g = wm.global_windows(x, ndims, W)
    b = wm.brute_global_windows(x, ndims, W)
    for k in ("min", "max", "sum", "count"):
        assert np.array_equal(g[k].astype(np.int64), np.array(b[k], np.int64)), k
    kw, f = wm.kernel_window(chunk_len, ndims, W)
    assert kw % 8 == 0 and kw >= 8
    folded = wm.fold(wm.chunk_windows(x, chunk_len, ndims, kw), n, chunk_len, ndims, W)
    for k in ("min", "max", "sum"):
        assert np.array_equal(folded[k].astype(np.int64), g[k].astype(np.int64)), k
    ok = g["count"] > 0
    assert np.allclose(g["mean"][ok], g["sum"][ok] / g["count"][ok])


def test_model_refuses_shapes_without_global_windows():
    assert wm.kernel_window(1024, 80, 32) is None          # cfg3 at 1 KB: rows of 80 do not divide 1 024 elements
    assert wm.kernel_window(640, 8, 24) is None            # R = 80: neither a multiple nor a divisor of 24
    assert wm.kernel_window(640, 8, 16) == (16, 1)
    assert wm.kernel_window(640, 8, 160) == (80, 2)
