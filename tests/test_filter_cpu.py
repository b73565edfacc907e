"""CPU tests of filter rows (sprintz_mi355x_filter_rows, sprintz_mi355x_filter_row_ids): every validation return comes before the
device is touched, the constants and bindings are there, and the numpy model the GPU tier compares with (tests/filter_model.py)
equals a one-element-at-a-time brute force of the definition on ragged shapes."""

import numpy as np
import pytest

import filter_model as fm
from fixtures import buf_fixture, lib  # noqa: F401  (fixtures)


buf = buf_fixture(4096)


def test_constants_and_bindings(lib):
    import re
    import os
    assert (lib.FILTER_ALL, lib.FILTER_ANY) == (0, 1) == (fm.ALL, fm.ANY)
    assert "sprintz_mi355x_filter_rows" in lib.EXPORTED_SYMBOLS and "sprintz_mi355x_filter_row_ids" in lib.EXPORTED_SYMBOLS
    assert len(lib.filter_rows.argtypes) == 15 and len(lib.filter_row_ids.argtypes) == 8
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sprintz_mi355x.h")).read()
    assert re.search(r"#define SPRINTZ_FILTER_ALL 0u", hdr) and re.search(r"#define SPRINTZ_FILTER_ANY 1u", hdr)
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    from sprintz_amd import ChunkedCodec
    assert callable(ChunkedCodec.filter_rows)


def test_filter_rows_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=5120, D=8, lo=p, hi=p + 64, mode=0, flags=0, mask=p + 128, counts=p + 1024, rets=p + 2048)

    def call(**kw):
        a = dict(good, **kw)
        return lib.filter_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["lo"], a["hi"], a["mode"], a["flags"],
                               a["mask"], a["counts"], a["rets"], None)

    assert call(mode=2) == E.E_INVALID                                # unknown mode
    assert call(flags=2) == E.E_INVALID and call(flags=3) == E.E_INVALID   # unknown flag (GENERAL_LAYOUT = 1 is the only one)
    for k in ("lo", "hi", "comp", "offs"):
        assert call(**{k: None}) == E.E_INVALID, k                    # NULL inputs
    assert call(mask=None, counts=None) == E.E_INVALID                # both outputs NULL
    assert call(lo=p + 1) == E.E_INVALID and call(hi=p + 65) == E.E_INVALID   # bounds not aligned to the element size
    assert call(counts=p + 1026) == E.E_INVALID                       # counts not aligned to 4 bytes
    assert call(rets=p + 2052) == E.E_INVALID                         # rets not aligned to 8 bytes
    assert call(D=0) == E.E_INVALID and call(cl=0) == E.E_INVALID and call(codec=9) == E.E_INVALID and call(esz=3) == E.E_INVALID
    assert call(D=513) == E.E_UNSUPPORTED                             # more than 512 columns
    for codec in (2, 3):
        assert call(codec=codec) == E.E_UNSUPPORTED                   # the non-RLE codecs
    assert call(codec=4, esz=1) == E.E_UNSUPPORTED
    assert "filter_rows" in lib.last_error()
    assert call(n=0) == 0                                             # nothing to do: returns 0, launches nothing
    # an odd address is fine for 8-bit bounds; either output alone is fine: such calls get as far as the device
    import torch
    if not torch.cuda.is_available():
        assert call() == E.E_NO_DEVICE
        assert call(esz=1, lo=p + 1, hi=p + 3) == E.E_NO_DEVICE
        assert call(mask=None) == E.E_NO_DEVICE and call(counts=None) == E.E_NO_DEVICE and call(rets=None) == E.E_NO_DEVICE
        assert call(flags=1, D=512) == E.E_NO_DEVICE


def test_filter_row_ids_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    assert lib.filter_row_ids(p, p + 64, 3, 5121, 8, p + 128, 10, None) == E.E_INVALID      # chunk_len % ndims
    assert lib.filter_row_ids(p, p + 64, 3, 5120, 0, p + 128, 10, None) == E.E_INVALID      # ndims == 0
    assert lib.filter_row_ids(p, p + 64, 3, 0, 8, p + 128, 10, None) == E.E_INVALID
    assert lib.filter_row_ids(None, p + 64, 3, 5120, 8, p + 128, 10, None) == E.E_INVALID   # NULL pointers with chunks
    assert lib.filter_row_ids(p, None, 3, 5120, 8, p + 128, 10, None) == E.E_INVALID
    assert lib.filter_row_ids(p, p + 64, 3, 5120, 8, None, 10, None) == E.E_INVALID
    assert lib.filter_row_ids(p, p + 68, 3, 5120, 8, p + 128, 10, None) == E.E_INVALID      # misaligned bases
    assert lib.filter_row_ids(p, p + 64, 3, 5120, 8, p + 132, 10, None) == E.E_INVALID      # misaligned ids
    assert lib.filter_row_ids(None, None, 0, 5120, 8, None, 0, None) == 0                   # no chunks: nothing to do
    assert lib.filter_row_ids(p + 1, p + 64, 0, 5120, 8, p + 128, 10, None) == 0
    import torch
    if not torch.cuda.is_available():
        assert lib.filter_row_ids(p + 1, p + 64, 3, 5120, 8, p + 128, 0, None) == E.E_NO_DEVICE   # the mask may lie anywhere


RAGGED = [
    # (esz, D, chunk_len, n): chunk_len % D != 0, a short last chunk ending mid-row, R % 8 != 0
    (1, 3, 100, 100 * 4 + 41),
    (2, 5, 83, 83 * 3 + 17),
    (1, 1, 13, 13 * 5 + 6),
    (2, 8, 8 * 21, 8 * 21 * 3 + 8 * 5 + 3),
    (1, 7, 7 * 16 + 2, (7 * 16 + 2) * 2 + 7 * 9 + 6),
    (2, 2, 64, 64 * 4),
]


@pytest.mark.parametrize("esz,D,chunk_len,n", RAGGED)
@pytest.mark.parametrize("mode", [fm.ALL, fm.ANY])
def test_model_equals_brute_force(esz, D, chunk_len, n, mode):
    rng = np.random.default_rng(n * 31 + D + mode)
    top = (1 << (8 * esz)) - 1
    x = rng.integers(0, top + 1, n)
    x[rng.integers(0, n, n // 8)] = 0
    x[rng.integers(0, n, n // 8)] = top
    for trial in range(6):
        lo = rng.integers(0, top + 1, D)
        hi = rng.integers(0, top + 1, D)
        if trial == 0:
            lo[:], hi[:] = fm.neutral(esz, mode)
        elif trial == 1:
            lo[:], hi[:] = fm.neutral(esz, 1 - mode)
        elif trial < 4:                                 # wide intervals: most columns match
            lo, hi = np.minimum(lo, hi) // 4, top - (top - np.maximum(lo, hi)) // 4
        got, want = fm.filter_rows(x, chunk_len, D, lo, hi, mode), fm.filter_rows_brute(x, chunk_len, D, lo, hi, mode)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (trial, lo, hi)
        R, MB = fm.geometry(chunk_len, D)
        assert got[0].shape == (-(-n // chunk_len), MB)
        assert np.array_equal(np.unpackbits(got[0], axis=1, bitorder="little").sum(axis=1), got[1])
        if trial == 0:                                  # neutral bounds: every existing row under ALL, none under ANY
            rows = [ne // D for ne in fm.chunk_counts(n, chunk_len)]
            assert list(got[1]) == (rows if mode == fm.ALL else [0] * len(rows))


def test_model_row_ids():
    rng = np.random.default_rng(3)
    D, chunk_len = 4, 4 * 21                             # R = 21: the last mask byte of a chunk is partly padding
    x = rng.integers(0, 256, chunk_len * 5 + 4 * 7)
    mask, counts = fm.filter_rows(x, chunk_len, D, [0, 0, 0, 0], [99, 255, 255, 255], fm.ALL)
    want = np.flatnonzero(x[: x.size // D * D].reshape(-1, D)[:, 0] <= 99)
    ids = fm.row_ids(mask, chunk_len, D)
    assert np.array_equal(ids, want) and ids.size == counts.sum()
    cut = fm.row_ids(mask, chunk_len, D, capacity=ids.size + 5, sentinel=-7)
    assert np.array_equal(cut[:ids.size], ids) and np.all(cut[ids.size:] == -7)
    assert np.array_equal(fm.row_ids(mask, chunk_len, D, capacity=3), ids[:3])
