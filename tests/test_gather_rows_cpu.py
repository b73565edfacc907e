"""CPU tests of gather rows (sprintz_mi355x_gather_rows): every refusal happens before a device is needed, and the numpy
model of its piece arithmetic (tests/gather_model.py) agrees with a row-by-row loop on the edge shapes."""
import ctypes as C
import os

import numpy as np
import pytest

import gather_model as gm
from fixtures import lib  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gather_rows_validation(lib):
    buf = (C.c_uint8 * 8192)()
    p = (C.addressof(buf) + 15) & ~15
    E = lib

    def g(codec=1, esz=2, comp=p, offs=p, n=1, chunk_len=640, D=8, starts=p + 1024, nranges=4, rows=16, out=p + 2048, rets=None):
        return lib.gather_rows(codec, esz, comp, offs, n, chunk_len, D, starts, nranges, rows, out, rets, None)

    # check_common
    assert g(codec=9) == E.E_INVALID
    assert g(codec=-1) == E.E_INVALID
    assert g(esz=3) == E.E_INVALID
    assert g(D=0) == E.E_INVALID
    assert g(codec=4, esz=2) == E.E_UNSUPPORTED                                   # xff_norle is 8-bit only
    # the non-RLE codecs
    for codec in (2, 3):
        assert g(codec=codec) == E.E_UNSUPPORTED, codec
    assert g(codec=4, esz=1) == E.E_UNSUPPORTED
    # more than 512 columns
    assert g(D=513, chunk_len=513 * 16) == E.E_UNSUPPORTED
    assert g(D=4096, chunk_len=4096 * 16) == E.E_UNSUPPORTED
    # rows must not straddle chunks
    assert g(chunk_len=641) == E.E_INVALID
    assert g(D=3, chunk_len=100) == E.E_INVALID
    # rows == 0
    assert g(rows=0) == E.E_INVALID
    # chunk_len in 1 .. 2^30
    assert g(chunk_len=0) == E.E_INVALID
    assert g(chunk_len=(1 << 30) + 8) == E.E_INVALID
    assert g(chunk_len=0xfffffff8) == E.E_INVALID
    # null pointers
    assert g(comp=None) == E.E_INVALID
    assert g(offs=None) == E.E_INVALID
    assert g(out=None) == E.E_INVALID
    assert g(starts=None) == E.E_INVALID
    assert g(starts=None, nranges=1) == E.E_INVALID
    # alignment: d_out to the element size, d_starts / d_rets to 8 bytes
    assert g(out=p + 2049) == E.E_INVALID
    assert g(starts=p + 1028) == E.E_INVALID
    assert g(starts=p + 1025) == E.E_INVALID
    assert g(rets=p + 4100) == E.E_INVALID
    assert g(rets=p + 4097) == E.E_INVALID

    import torch
    if torch.cuda.is_available():
        return
    # valid arguments reach the device check
    assert g() == E.E_NO_DEVICE
    assert g(esz=1, out=p + 2049, codec=0) == E.E_NO_DEVICE                       # 8-bit elements: any d_out
    assert g(out=p + 2050) == E.E_NO_DEVICE                                       # element-aligned is enough
    assert g(rets=p + 4096) == E.E_NO_DEVICE
    assert g(starts=None, nranges=0) == E.E_NO_DEVICE                             # no ranges: no starts needed
    assert g(D=512, chunk_len=512 * 16, rows=1) == E.E_NO_DEVICE
    assert g(D=1, esz=1, codec=0, chunk_len=1 << 30, rows=0xffffffff) == E.E_NO_DEVICE
    assert g(chunk_len=8, rows=100000) == E.E_NO_DEVICE                           # one row a chunk, 100 000 chunks a range
    assert "no CPU fallback" in lib.last_error() or lib.last_error()


def test_gather_rows_binding(lib):
    assert "sprintz_mi355x_gather_rows" in lib.EXPORTED_SYMBOLS
    assert lib.abi_version() == 7                                                 # additive: the version stays
    text = open(os.path.join(ROOT, "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_gather_rows(" in text
    import sprintz_amd
    assert callable(sprintz_amd.ChunkedCodec.gather_rows) and callable(sprintz_amd.ChunkedCodec.read_rows)


def brute_pieces(start, rows, R, nchunks, srows):
    """row by row: where does row r of the range come from?"""
    ps, ok = [], True
    for r in range(rows):
        g = start + r
        c, cr = divmod(g, R)
        if c >= nchunks or cr >= srows[c]:
            ok = False
            continue
        if ps and ps[-1][0] == c and ps[-1][2] == cr and ps[-1][3] + ps[-1][2] - ps[-1][1] == r:
            ps[-1] = (c, ps[-1][1], cr + 1, ps[-1][3])
        else:
            ps.append((c, cr, cr + 1, r))
    return ps, ok


@pytest.mark.parametrize("R,nchunks,last_rows", [(40, 6, 40), (40, 6, 13), (16, 9, 1), (1, 30, 1), (7, 5, 3), (640, 4, 300)])
def test_model_pieces_match_brute_force(R, nchunks, last_rows):
    srows = np.full(nchunks, R, np.int64)
    srows[-1] = last_rows
    total = (nchunks - 1) * R + last_rows
    for rows in sorted({1, max(1, R - 1), R, R + 1, 3 * R + 5}):
        starts = {0, total - 1, total, total + 5 * R + 3, max(0, total - rows), max(0, total - rows - 1), max(0, total - rows + 1)}
        for c in range(1, nchunks + 1):
            starts |= {c * R - 1, c * R, c * R + 1}
        starts = sorted(s for s in starts if s >= 0)
        got, rets = gm.pieces(starts, rows, R, nchunks, srows)
        P = gm.max_pieces(rows, R)
        for s, ps, ret in zip(starts, got, rets):
            want, ok = brute_pieces(s, rows, R, nchunks, srows)
            # a short chunk in the MIDDLE of a range cannot happen here (only the last chunk is short): same pieces
            assert ps == want, (R, rows, s, ps, want)
            assert ret == (rows if ok else gm.E_INVALID), (R, rows, s)
            assert len(ps) <= P, (R, rows, s, len(ps), P)
            assert all(0 <= lo < hi <= R for _, lo, hi, _ in ps)
            if ok:                                             # the pieces tile [0, rows) exactly once, on consecutive chunks
                cover = np.zeros(rows, np.int64)
                for c, lo, hi, o in ps:
                    cover[o:o + hi - lo] += 1
                assert np.all(cover == 1), (R, rows, s)
                assert [p[0] for p in ps] == list(range(ps[0][0], ps[0][0] + len(ps)))
                assert ps[0][0] == s // R and ps[0][1] == s % R and ps[0][3] == 0
        # P is reached: a range that starts on a chunk's last row
        if nchunks * R >= rows + R:
            ps, _ = gm.pieces([R - 1], rows, R, nchunks + P, np.full(nchunks + P, R))
            assert len(ps[0]) == P, (R, rows)


def test_model_expected_slices_the_input():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 65536, (1000, 8)).astype(np.uint16)
    starts = [0, 5, 990, 995, 1000, 4000, 5]
    out, ok = gm.expected(x, starts, 10)
    assert ok.tolist() == [True, True, True, False, False, False, True]
    assert np.array_equal(out[1], x[5:15]) and np.array_equal(out[6], out[1]) and np.array_equal(out[2], x[990:])
    assert np.array_equal(out[3][:5], x[995:]) and not out[3][5:].any() and not out[4].any()
    flat, ok2 = gm.expected(x.ravel()[:-3], starts, 10, ndims=8)                 # a partial last row is no row
    assert ok2.tolist() == [True, True, False, False, False, False, True]
    assert np.array_equal(gm.stream_rows(8 * 1000 - 3, 640, 8), [80] * 12 + [39])
