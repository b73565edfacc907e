"""CPU tests of extrema rows (sprintz_mi355x_extrema_rows): the symbol and its binding are there, every validation return comes before
the device is touched and names the operation, the numpy model the GPU tier compares with (tests/extrema_model.py) equals brute force
and satisfies the identities that tie it to aggregate rows and to plain indexing, rowops.fold_extrema folds per-chunk windows into the
model's windows over the batch's rows, and the planner (sprintz_amd/csrc/plan.h, built with g++: tests/plan_probe.cpp) sends the
mode to decode_fast.h exactly where aggregate rows go, to the generic kernel otherwise -- never to decode_uni.h or the plain decode's
kernels.  The kernels keep value and row apart, so there is no window limit to probe."""
import os

import numpy as np
import pytest

import aggregate_model as am
import extrema_model as em
import filter_model as fm
from fixtures import buf_fixture, lib, random_mask, refusals  # noqa: F401  (fixtures)
from planner import QUERY, plan_fixture, split

HERE = os.path.dirname(os.path.abspath(__file__))
Q_WINDOW, Q_AGGREGATE, Q_EXTREMA = QUERY["window"], QUERY["aggregate"], QUERY["extrema"]


buf = buf_fixture(65536)


def test_symbol_and_binding(lib):
    assert "sprintz_mi355x_extrema_rows" in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.lib, "sprintz_mi355x_extrema_rows")
    assert len(lib.extrema_rows.argtypes) == 21
    assert (lib.EXT_MIN, lib.EXT_MAX, lib.EXT_ARGMIN, lib.EXT_ARGMAX, lib.EXT_FIRST, lib.EXT_LAST, lib.EXT_ROWS, lib.EXT_COUNT) == \
        (1, 2, 4, 8, 16, 32, 64, 128)
    assert lib.EXT_NO_ROW == 0xFFFFFFFF == em.NO_ROW
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_extrema_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    assert "uint32_t flags, void* d_min, void* d_max, uint32_t* d_argmin, uint32_t* d_argmax," in hdr
    assert "void* d_first, void* d_last, uint32_t* d_rows, uint32_t* d_count, int64_t* d_rets," in hdr
    for name, v in (("MIN", 1), ("MAX", 2), ("ARGMIN", 4), ("ARGMAX", 8), ("FIRST", 16), ("LAST", 32), ("ROWS", 64), ("COUNT", 128)):
        assert f"#define SPRINTZ_EXT_{name} {v}u" in hdr
    assert "#define SPRINTZ_EXT_NO_ROW 0xFFFFFFFFu" in hdr
    assert "extrema_rows, SPRINTZ_EXT_*" in hdr                   # the ABI-history comment
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    from sprintz_amd import ChunkedCodec
    assert callable(ChunkedCodec.extrema_rows) and callable(ChunkedCodec.extrema_where) and callable(ChunkedCodec.m4)


OUTS = ("min", "max", "argmin", "argmax", "first", "last", "rows", "count")       # in the order of their op bits


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=5120, D=8, mask=p + 128, W=64, ops=255, flags=0, min=p + 2048, max=p + 4096,
                argmin=p + 6144, argmax=p + 8192, first=p + 10240, last=p + 12288, rows=p + 14336, count=p + 16384, rets=p + 32768)

    def call(**kw):
        a = dict(good, **kw)
        return lib.extrema_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["mask"], a["W"], a["ops"], a["flags"],
                                *[a[k] for k in OUTS], a["rets"], None)

    invalid, unsupported = refusals(lib, call, "extrema_rows")

    invalid(cl=5121)                                                             # chunk_len % ndims != 0
    invalid(D=7)
    invalid(cl=0)                                                                # chunk_len outside 1..2^30
    invalid(cl=(1 << 30) + 8)
    for W in (0, 4, 7, 9, 12, 63, 65, 0xFFFFFFFF):                               # window_rows: a multiple of 8, at least 8
        invalid(W=W)
    for ops in (0, 256, 257, 511, 0x80000001, 0xFFFFFFFF):                       # ops outside 1..255
        invalid(ops=ops)
    for i, k in enumerate(OUTS):                                                 # a selected output that is NULL
        invalid(**{k: None})
        invalid(ops=1 << i, **{k: None})
    for k in ("comp", "offs"):                                                   # NULL d_comp / d_offsets
        invalid(**{k: None})
    for k in ("min", "max", "first", "last"):                                    # not aligned to the element size
        invalid(**{k: good[k] + 1})
    for k in ("argmin", "argmax", "rows", "count"):                              # not aligned to 4 bytes
        for off in (1, 2, 3):
            invalid(**{k: good[k] + off})
    for off in (1, 2, 4):                                                        # d_rets not aligned to 8 bytes
        invalid(rets=good["rets"] + off)
    invalid(flags=2)                                                             # unknown flag (GENERAL_LAYOUT = 1 is the only one)
    invalid(flags=3)
    assert call(D=0) == E.E_INVALID and call(codec=9) == E.E_INVALID and call(esz=3) == E.E_INVALID
    unsupported(D=513, cl=513 * 16)                                              # more than 512 columns
    for codec in (2, 3):
        unsupported(codec=codec)                                                 # the non-RLE codecs
    unsupported(codec=4, esz=1)
    assert call(n=0) == 0                                                        # nothing to do: returns 0, launches nothing
    assert call(n=0, mask=None, rets=None) == 0
    import torch
    if not torch.cuda.is_available():
        assert call() == E.E_NO_DEVICE
        assert call(mask=None) == E.E_NO_DEVICE and call(rets=None) == E.E_NO_DEVICE      # a NULL mask: every row
        assert call(mask=p + 129) == E.E_NO_DEVICE                               # the mask may lie anywhere
        for i, k in enumerate(OUTS):                                             # an unselected output may be NULL, or lie anywhere
            assert call(ops=255 & ~(1 << i), **{k: None}) == E.E_NO_DEVICE, k
            assert call(ops=255 & ~(1 << i), **{k: good[k] + 1}) == E.E_NO_DEVICE, k
            assert call(ops=1 << i) == E.E_NO_DEVICE                             # each op alone
            assert call(ops=1 << i, **{o: None for o in OUTS if o != k}) == E.E_NO_DEVICE, k
        for ops in (1, 128, 255, 4 | 8, 16 | 32 | 64):
            assert call(ops=ops) == E.E_NO_DEVICE
        assert call(ops=4, min=None) == E.E_NO_DEVICE and call(ops=8, max=None) == E.E_NO_DEVICE     # ARGMIN without MIN is legal
        assert call(esz=1, min=good["min"] + 1, first=good["first"] + 3) == E.E_NO_DEVICE            # one-byte elements lie anywhere
        assert call(D=512, cl=512 * 16) == E.E_NO_DEVICE and call(D=512, cl=512 * 16, flags=1) == E.E_NO_DEVICE
        for W in (8, 16, 640, 648, 1 << 20, 0xFFFFFFF8):
            assert call(W=W) == E.E_NO_DEVICE
        assert call(codec=0) == E.E_NO_DEVICE and call(cl=1 << 30) == E.E_NO_DEVICE


SHAPES = [
    # test_groupby_cpu.py's: (esz, D, chunk_len, n): whole rows and short last chunks (one ending mid-row), R % 8 != 0 and R < 8
    (1, 3, 3 * 33, 3 * 33 * 4 + 3 * 14),
    (2, 5, 5 * 21, 5 * 21 * 3 + 5 * 4 + 2),
    (1, 1, 13, 13 * 5 + 6),
    (2, 8, 8 * 64, 8 * 64 * 3),
    (1, 7, 7 * 5, 7 * 5 * 6 + 7),
]
KEYS = ("min", "max", "argmin", "argmax", "first", "last", "rows", "count")


def windows_of(R):
    r8 = -(-R // 8) * 8
    return sorted({8, 24, r8, r8 + 8})


def check_identities(x, chunk_len, D, mask, W, got):
    """what ties the model to aggregate rows and to plain indexing"""
    R = chunk_len // D
    nwin = -(-R // W)
    nchunks = got["count"].shape[0]
    full = np.full((nchunks, -(-R // 8)), 0xFF, np.uint8) if mask is None else mask
    agg = am.aggregate_rows(x, chunk_len, D, full, W)
    for k in ("min", "max", "count"):
        assert np.array_equal(got[k], agg[k]), k
    sel = em.selected(mask, x.size, chunk_len, D)
    for c in range(nchunks):
        rows = x[c * chunk_len:(c + 1) * chunk_len]
        rows = rows[:rows.size // D * D].reshape(-1, D)
        for w in range(nwin):
            s = np.flatnonzero(sel[c, w * W:(w + 1) * W]) + w * W
            if s.size == 0:
                assert (got["argmin"][c, w] == em.NO_ROW).all() and (got["argmax"][c, w] == em.NO_ROW).all() and (got["rows"][c, w] == em.NO_ROW).all()
                assert not got["first"][c, w].any() and not got["last"][c, w].any() and got["count"][c, w] == 0
                assert (got["min"][c, w] == am.ident_min(x.dtype.itemsize)).all() and not got["max"][c, w].any()
                continue
            assert tuple(got["rows"][c, w]) == (s[0], s[-1])
            assert np.array_equal(got["first"][c, w], rows[s[0]]) and np.array_equal(got["last"][c, w], rows[s[-1]])
            for d in range(D):
                for arg, val in (("argmin", "min"), ("argmax", "max")):
                    r = int(got[arg][c, w, d])
                    assert r in s and rows[r, d] == got[val][c, w, d]            # x[argmin] is the min, in a selected row of the window ...
                    assert not (rows[s[s < r], d] == got[val][c, w, d]).any()    # ... and no earlier selected row holds it


@pytest.mark.parametrize("esz,D,chunk_len,n", SHAPES)
def test_model_equals_brute_force(esz, D, chunk_len, n):
    rng = np.random.default_rng(n + D)
    x = rng.integers(0, 1 << (8 * esz), n).astype(np.uint8 if esz == 1 else np.uint16)
    R, MB = fm.geometry(chunk_len, D)
    nchunks = -(-n // chunk_len)
    for p in (None, 0.0, 0.3, 1.0):
        mask = None if p is None else random_mask(rng, nchunks, MB, p)     # bits of rows that do not exist are set too: they are ignored
        for W in windows_of(R):
            got = em.extrema_rows(x, chunk_len, D, mask, W)
            brute = em.extrema_rows_brute(x, chunk_len, D, mask, W)
            nwin = -(-R // W)
            for k in KEYS:
                assert got[k].dtype == brute[k].dtype == (x.dtype if k in ("min", "max", "first", "last") else np.uint32), k
                assert got[k].shape == ((nchunks, nwin) if k == "count" else (nchunks, nwin, 2) if k == "rows" else (nchunks, nwin, D)), k
                assert np.array_equal(got[k], brute[k]), (p, W, k)
            check_identities(x, chunk_len, D, mask, W, got)
            if p == 0.0:
                assert not got["count"].any() and (got["argmin"] == em.NO_ROW).all()


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("kind", ["constant", "two_valued", "extremes"])
def test_model_ties(esz, kind):
    """the first occurrence wins: constant data, two values, and the identities' own values (0 and all ones) as data"""
    rng = np.random.default_rng(esz)
    D, R, nchunks = 3, 40, 3
    chunk_len, n = D * R, D * R * nchunks - D * 7
    top = (1 << (8 * esz)) - 1
    dt = np.uint8 if esz == 1 else np.uint16
    x = (np.full(n, 77) if kind == "constant" else rng.integers(0, 2, n) * 5 + 9 if kind == "two_valued" else rng.integers(0, 2, n) * top).astype(dt)
    for p in (None, 0.4):
        mask = None if p is None else random_mask(rng, nchunks, 5, p)
        for W in (8, 16, 40):
            got = em.extrema_rows(x, chunk_len, D, mask, W)
            brute = em.extrema_rows_brute(x, chunk_len, D, mask, W)
            for k in KEYS:
                assert np.array_equal(got[k], brute[k]), (p, W, k)
            check_identities(x, chunk_len, D, mask, W, got)
            if kind == "constant":                                                # every position is the window's first selected row
                assert np.array_equal(got["argmin"], np.repeat(got["rows"][..., :1], D, axis=2)) and np.array_equal(got["argmin"], got["argmax"])


def per_chunk_as_torch(x, chunk_len, D, mask, kw):
    """the model's per-chunk windows in the form ChunkedCodec.extrema_rows hands to rowops.fold_extrema: rows as int64 batch rows, -1: none"""
    import torch
    R = chunk_len // D
    m = em.extrema_rows(x, chunk_len, D, mask, kw)
    n = m["count"].shape[0]
    base = (np.arange(n, dtype=np.int64) * R).reshape(n, 1, 1)
    rows = lambda v: np.where(v == em.NO_ROW, -1, v.astype(np.int64) + base)
    dt = torch.uint8 if x.dtype == np.uint8 else torch.uint16
    view = np.int8 if x.dtype == np.uint8 else np.int16
    res = {k: torch.from_numpy(m[k].view(view).copy()).view(dt) for k in ("min", "max", "first", "last")}
    res.update({k: torch.from_numpy(rows(m[k])) for k in ("argmin", "argmax")})
    fl = rows(m["rows"])
    res["first_row"], res["last_row"] = torch.from_numpy(fl[..., 0].copy()), torch.from_numpy(fl[..., 1].copy())
    res["count"] = torch.from_numpy(m["count"].astype(np.int64))
    return res, dt


def as_numpy(t, dtype):
    import torch
    if t.dtype in (torch.uint8, torch.uint16):
        return t.view(torch.int8 if t.dtype == torch.uint8 else torch.int16).numpy().view(dtype)
    return t.numpy()


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("fold", [1, 2, 3])
def test_fold_extrema(esz, fold):
    """rowops.fold_extrema against the model's windows over the batch's rows: fold chunks a window, a batch whose last window lacks
    chunks, and -- two-valued data -- windows whose minimum and maximum tie across chunks"""
    from sprintz_amd import rowops
    rng = np.random.default_rng(10 * esz + fold)
    D, R, nchunks = 3, 24, 7                                                      # 7 chunks: the last window of fold 2 / 3 lacks one / two
    chunk_len = D * R
    n = chunk_len * (nchunks - 1) + D * 11 + 1                                    # a short last chunk that ends mid-row
    dt = np.uint8 if esz == 1 else np.uint16
    top = (1 << (8 * esz)) - 1
    for kind in ("random", "two_valued", "extremes"):
        x = (rng.integers(0, top + 1, n) if kind == "random" else rng.integers(0, 2, n) * 3 + 4 if kind == "two_valued" else rng.integers(0, 2, n) * top).astype(dt)
        for p in (None, 0.0, 0.15, 1.0):
            mask = None if p is None else random_mask(rng, nchunks, 3, p)
            if p == 0.15:
                mask[2] = 0                                                       # a chunk with no selected row inside a window
            for W in ([R * fold] if fold > 1 else [R, 8]):
                kw, f, nwin = rowops.plan_windows(R, W, False)
                assert f == fold and kw % 8 == 0
                res, tdt = per_chunk_as_torch(x, chunk_len, D, mask, kw)
                got = rowops.fold_extrema(res, nchunks, nwin, D, W, fold, n, esz, tdt)
                want = em.global_windows(x, chunk_len, D, mask, W)
                assert set(got) == set(want)
                for k, v in want.items():
                    g = as_numpy(got[k], dt)
                    assert g.shape == v.shape and np.array_equal(g, v), (kind, p, W, k)
                # a subset: the fold takes what it is given
                sub = rowops.fold_extrema({k: res[k] for k in ("max", "argmax", "count")}, nchunks, nwin, D, W, fold, n, esz, tdt)
                assert set(sub) == {"max", "argmax", "count"} and np.array_equal(sub["argmax"].numpy(), want["argmax"])


def test_fold_extrema_tie_across_chunks():
    """the window's minimum stands in two chunks: the position is the first chunk's; an empty chunk in front holds the identity -- all
    ones, which is also a value -- and must not win"""
    import torch
    from sprintz_amd import rowops
    D, R = 1, 8
    x = np.array([0xFFFF] * 8 + [0xFFFF, 7, 9, 7, 9, 9, 9, 9] + [9, 9, 7, 9, 9, 9, 9, 0xFFFF], np.uint16)
    mask = np.array([[0x00], [0xFF], [0xFF]], np.uint8)
    res, tdt = per_chunk_as_torch(x, 8, 1, mask, 8)
    got = rowops.fold_extrema(res, 3, 1, 1, 24, 3, 24, 2, tdt)
    assert got["argmin"].tolist() == [[9]] and got["argmax"].tolist() == [[8]] and got["first_row"].tolist() == [8] and got["last_row"].tolist() == [23]
    assert as_numpy(got["min"], np.uint16).tolist() == [[7]] and as_numpy(got["max"], np.uint16).tolist() == [[0xFFFF]]
    mask = np.array([[0x00], [0x01], [0x80]], np.uint8)                           # only rows 8 and 23, both all ones: the identity as a value
    res, tdt = per_chunk_as_torch(x, 8, 1, mask, 8)
    got = rowops.fold_extrema(res, 3, 1, 1, 24, 3, 24, 2, tdt)
    assert got["argmin"].tolist() == [[8]] and got["argmax"].tolist() == [[8]] and got["count"].tolist() == [2]
    assert as_numpy(got["first"], np.uint16).tolist() == [[0xFFFF]] and got["last_row"].tolist() == [23]


plan = plan_fixture(shape=split, codec=1, nchunks=4096, q=Q_EXTREMA)


PLAN_SHAPES = [(1, 16, 16 * 512), (2, 8, 5120), (2, 24, 24 * 200), (1, 8, 4096), (2, 4, 4096), (1, 24, 24 * 200), (2, 5, 5 * 1024), (2, 3, 3000),
               (1, 80, 10240), (2, 128, 128 * 80), (1, 256, 256 * 80), (2, 300, 9600), (1, 512, 512 * 16), (2, 33, 33 * 64), (1, 5, 5 * 1024),
               (1, 33, 33 * 128), (2, 8, 8 * 13), (1, 1, 1024), (2, 1, 1024), (1, 2, 2048), (2, 2, 2048), (1, 3, 3000), (1, 4, 4096),
               (2, 8, 8 * 65536), (2, 8, 8 * 65544), (1, 8, 8 << 24), (1, 8, (8 << 24) + 64)]


def test_planner(plan):
    families = set()
    for esz, D, cl in PLAN_SHAPES:
        for codec in (0, 1):
            for general in (0, 1):
                for no_fast in (0, 1):
                    kw = dict(esz=esz, D=D, chunk_len=cl, codec=codec, general=general, no_fast=no_fast)
                    ext, agg = plan(**kw), plan(q=Q_AGGREGATE, **kw)
                    assert ext == agg, kw                    # the family, the launch's LDS, the grid and the mapping are aggregate's: no window limit
                    assert ext[0] in ("dec_fast", "dec_generic"), kw
                    assert not (no_fast and ext[0] == "dec_fast")
                    families.add(ext[0])
    assert families == {"dec_fast", "dec_generic"}
    assert plan(esz=2, D=8, chunk_len=5120)[0] == "dec_fast" and plan(esz=2, D=8, chunk_len=5120, codec=0)[0] == "dec_fast"
    # the low-dimension layouts: decode_uni.h serves the windowed query and is not taught this mode
    for esz, D, cl in [(1, 1, 1024), (2, 1, 1024), (1, 2, 2048), (2, 2, 2048), (1, 3, 3000), (1, 4, 4096)]:
        assert plan(esz=esz, D=D, chunk_len=cl, q=Q_WINDOW)[0] == "dec_uni", (esz, D, cl)
        assert plan(esz=esz, D=D, chunk_len=cl)[0] == "dec_generic", (esz, D, cl)
    # the mode never reaches the small-batch, row, block-parallel or univariate kernels, whatever the batch size and the knobs
    for nchunks in (1, 2, 64, 2048, 2049, 131072, 1 << 20):
        for codec in (0, 1):
            for blk in (0, 1, 4096):
                assert plan(esz=2, D=8, chunk_len=5120, nchunks=nchunks, codec=codec, blk_chunks=blk)[0] == "dec_fast"
                assert plan(esz=1, D=64, chunk_len=64 * 160, nchunks=nchunks, codec=codec, blk_chunks=blk)[0] == "dec_fast"
                assert plan(esz=1, D=1, chunk_len=1024, nchunks=nchunks, codec=codec, blk_chunks=blk)[0] == "dec_generic"
                assert plan(esz=2, D=2, chunk_len=2048, nchunks=nchunks, codec=codec, blk_chunks=blk)[0] == "dec_generic"


def test_planner_leaves_the_other_modes_alone(plan):
    """every other mode's plan is what the parent's planner gives: the only edit is the univariate kernel's list of modes it is not
    taught, which names mode 11 alone.  Pinned here as facts about those modes (their own CPU tests pin the rest)"""
    assert plan(esz=1, D=1, chunk_len=1024, q=5)[0] == "dec_uni" and plan(esz=1, D=1, chunk_len=1024, q=6)[0] == "dec_generic"
    for q in (0, 1, 2, 3, 5):
        assert plan(esz=1, D=1, chunk_len=1024, q=q, nchunks=1 << 16)[0] == "dec_uni", q
    for q in (6, 7, 8, 9, 10):
        assert plan(esz=1, D=1, chunk_len=1024, q=q, nchunks=1 << 16)[0] == "dec_generic", q
    assert plan(esz=2, D=8, chunk_len=5120, q=0, nchunks=64)[0] == "dec_lat"
    for q in (3, 7, 9):
        assert plan(esz=2, D=8, chunk_len=5120, q=q) == plan(esz=2, D=8, chunk_len=5120, q=Q_WINDOW), q
