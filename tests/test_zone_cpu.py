"""CPU tests of zone-map pruning (sprintz_mi355x_zone_map / _zone_prune_box / _zone_prune_linear / _zone_expand): the symbols and their
bindings are there, every validation return comes before the device is touched, the rules of sprintz_amd/csrc/zone.h (built with g++:
tests/zone_probe.cpp) equal the numpy model (tests/zone_model.py) on a grid of edge values, the model is SOUND against the filters' own
models on random chunks -- a NONE chunk has an all-zero mask, an ALL chunk exactly the bits of its rows -- and rowops' host reference of
classify and expand equals the model.  Every comparison is exact."""
import ctypes as C
import inspect
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import filter_model as fm
import linear_model as lm
import zone_model as zm
from harness import DTYPES
from fixtures import buf_fixture, lib  # noqa: F401  (fixtures)
from rowdata import weight_sets

HERE = os.path.dirname(os.path.abspath(__file__))


buf = buf_fixture(65536)


SYMBOLS = ("sprintz_mi355x_zone_map", "sprintz_mi355x_zone_prune_tmp_bytes", "sprintz_mi355x_zone_prune_box", "sprintz_mi355x_zone_prune_linear",
           "sprintz_mi355x_zone_expand")


def test_symbols_and_bindings(lib):
    for s in SYMBOLS:
        assert s in lib.EXPORTED_SYMBOLS and hasattr(lib.lib, s)
    assert [len(f.argtypes) for f in (lib.zone_map, lib.zone_prune_tmp_bytes, lib.zone_prune_box, lib.zone_prune_linear, lib.zone_expand)] == [12, 1, 16, 17, 13]
    assert lib.zone_prune_tmp_bytes.restype is C.c_size_t
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    for s in SYMBOLS:
        assert s + "(" in hdr
    assert "0xf0000000" in hdr and "THE 4 GiB RULE" in hdr                   # the span rule is the header's to state
    assert (lib.ZONE_NONE, lib.ZONE_ALL, lib.ZONE_DECODE) == (zm.NONE, zm.ALL, zm.DECODE) and lib.ZONE_SPAN_LIMIT == zm.SPAN_LIMIT
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33                     # additive: no new ABI version, no new kernel family
    zone_h = open(os.path.join(os.path.dirname(HERE), "sprintz_amd", "csrc", "zone.h")).read()
    assert "kZoneSpanLimit = 0xf0000000ull" in zone_h and "zone_span_too_wide" in zone_h     # the constant and the predicate live in the no-HIP header
    from sprintz_amd import ChunkedCodec, ZoneMap
    assert callable(ChunkedCodec.zone_map) and ZoneMap is not None
    for name in ("filter_rows", "filter_linear", "where", "aggregate_where"):
        assert "zones" in inspect.signature(getattr(ChunkedCodec, name)).parameters, name


def test_options_can_be_read_back(lib):
    """sprintz_mi355x_get_option is the library's own state: whoever set the option, through whichever binding"""
    assert "sprintz_mi355x_get_option" in lib.EXPORTED_SYMBOLS
    before = lib.ref_decoder_quirk()
    assert before in (0, 1) and before == lib.get_option(lib.OPT_REF_DECODER_QUIRK)
    try:
        assert lib.set_option(lib.OPT_REF_DECODER_QUIRK, 1) == 0 and lib.ref_decoder_quirk() == 1
        assert lib.lib.sprintz_mi355x_set_option(lib.OPT_REF_DECODER_QUIRK, 0) == 0 and lib.ref_decoder_quirk() == 0      # not through the binding's name
        assert lib.set_option(lib.OPT_REF_DECODER_QUIRK, 7) == 0 and lib.ref_decoder_quirk() == 1                        # any non-zero value is 1
        assert lib.set_option(99, 1) == lib.E_INVALID and lib.ref_decoder_quirk() == 1                                   # a refused call changes nothing
        assert lib.get_option(99) == lib.E_INVALID and lib.get_option(-1) == lib.E_INVALID and lib.last_error()
        for opt, v in ((lib.OPT_CHUNKS_PER_GROUP, 3), (lib.OPT_NO_FAST, 1), (lib.OPT_LAT_CHUNKS, 77), (lib.OPT_BLK_KERNELS, 5)):
            old = lib.get_option(opt)
            assert old >= 0 and lib.set_option(opt, v) == 0 and lib.get_option(opt) == v
            assert lib.set_option(opt, old) == 0 and lib.get_option(opt) == old
    finally:
        lib.set_option(lib.OPT_REF_DECODER_QUIRK, before)


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    import torch
    no_gpu = not torch.cuda.is_available()

    def checker(fn, order, good):
        def call(**kw):
            a = dict(good, **kw)
            return fn(*[a[k] for k in order])

        def invalid(**kw):
            assert call(**kw) == E.E_INVALID, kw
            assert lib.last_error(), kw
        return call, invalid

    # ---- zone_map: as query_windows, and its own three outputs
    order = ("codec", "esz", "comp", "offs", "n", "cl", "D", "flags", "zmin", "zmax", "zlen", "st")
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=5120, D=8, flags=0, zmin=p + 1024, zmax=p + 2048, zlen=p + 4096, st=None)
    call, invalid = checker(lib.zone_map, order, good)
    for k in ("comp", "offs", "zmin", "zmax", "zlen"):
        invalid(**{k: None})
    invalid(flags=2)
    invalid(cl=0)
    invalid(cl=(1 << 30) + 8)
    invalid(zmin=good["zmin"] + 1)                                               # min / max aligned to the element size
    invalid(zmax=good["zmax"] + 1)
    for off in (1, 2, 4):
        invalid(zlen=good["zlen"] + off)
    assert call(D=0) == E.E_INVALID and call(codec=9) == E.E_INVALID and call(esz=3) == E.E_INVALID
    assert call(D=513, cl=513 * 16) == E.E_UNSUPPORTED
    if no_gpu:
        assert call() == E.E_NO_DEVICE and call(flags=1) == E.E_NO_DEVICE and call(esz=1, zmin=good["zmin"] + 1) == E.E_NO_DEVICE
        assert call(cl=5123) == E.E_NO_DEVICE                                    # a partial last row is fine
        for codec in (2, 3):
            assert call(codec=codec) == E.E_NO_DEVICE                            # every codec query_windows takes

    # ---- zone_prune_box
    order = ("esz", "n", "cl", "D", "offs", "zmin", "zmax", "zlen", "lo", "hi", "mode", "cls", "pos", "surv", "tmp", "st")
    good = dict(esz=2, n=3, cl=5120, D=8, offs=p, zmin=p + 1024, zmax=p + 2048, zlen=p + 4096, lo=p + 128, hi=p + 256, mode=0, cls=p + 8192 + 1,
                pos=p + 12288, surv=p + 16384, tmp=p + 20480, st=None)
    call, invalid = checker(lib.zone_prune_box, order, good)
    for k in ("offs", "zmin", "zmax", "zlen", "lo", "hi", "cls", "pos", "surv", "tmp"):
        invalid(**{k: None})
    assert "zone_prune_box" in lib.last_error()
    invalid(mode=2)
    invalid(esz=0)
    invalid(esz=3)
    invalid(D=0)
    invalid(cl=0)
    invalid(cl=(1 << 30) + 8)
    for k in ("zmin", "zmax", "lo", "hi"):
        invalid(**{k: good[k] + 1})                                              # aligned to the element size
    for k in ("offs", "zlen", "pos", "surv", "tmp"):
        for off in (1, 2, 4):
            invalid(**{k: good[k] + off})                                        # aligned to 8 bytes
    assert call(D=513, cl=513 * 16) == E.E_UNSUPPORTED
    assert call(n=0) == 0                                                        # nothing to do: returns 0, launches nothing
    if no_gpu:
        assert call() == E.E_NO_DEVICE and call(mode=1) == E.E_NO_DEVICE and call(cl=5123) == E.E_NO_DEVICE
        assert call(esz=1, lo=good["lo"] + 1, zmin=good["zmin"] + 1) == E.E_NO_DEVICE
        assert call(D=512, cl=512 * 16) == E.E_NO_DEVICE

    # ---- zone_prune_linear
    order = ("esz", "n", "cl", "D", "offs", "zmin", "zmax", "zlen", "w", "bias", "lo", "hi", "cls", "pos", "surv", "tmp", "st")
    good = dict(esz=2, n=3, cl=5120, D=8, offs=p, zmin=p + 1024, zmax=p + 2048, zlen=p + 4096, w=p + 128, bias=0, lo=-5, hi=5, cls=p + 8192 + 1,
                pos=p + 12288, surv=p + 16384, tmp=p + 20480, st=None)
    call, invalid = checker(lib.zone_prune_linear, order, good)
    for k in ("offs", "zmin", "zmax", "zlen", "w", "cls", "pos", "surv", "tmp"):
        invalid(**{k: None})
    assert "zone_prune_linear" in lib.last_error()
    for off in (1, 2, 3):
        invalid(w=good["w"] + off)
    invalid(cl=5121)                                                             # chunk_len % ndims != 0
    invalid(D=7)
    invalid(D=0)
    invalid(esz=4)
    for k in ("offs", "zlen", "pos", "surv", "tmp"):
        invalid(**{k: good[k] + 4})
    assert call(D=513, cl=513 * 16) == E.E_UNSUPPORTED
    assert call(n=0) == 0
    if no_gpu:
        assert call() == E.E_NO_DEVICE and call(lo=5, hi=-5) == E.E_NO_DEVICE
        assert call(bias=-(1 << 31), lo=-(1 << 31), hi=(1 << 31) - 1) == E.E_NO_DEVICE

    # ---- zone_expand
    order = ("n", "cl", "D", "cls", "pos", "zlen", "cmask", "ccounts", "crets", "mask", "counts", "rets", "st")
    good = dict(n=3, cl=5120, D=8, cls=p + 1, pos=p + 1024, zlen=p + 2048, cmask=p + 4096 + 3, ccounts=p + 8192, crets=p + 12288, mask=p + 16384 + 1,
                counts=p + 20480, rets=p + 24576, st=None)
    call, invalid = checker(lib.zone_expand, order, good)
    for k in ("cls", "pos", "zlen"):
        invalid(**{k: None})
    assert "zone_expand" in lib.last_error()
    invalid(mask=None, counts=None)
    invalid(D=0)
    invalid(cl=0)
    invalid(cl=(1 << 30) + 8)
    for k in ("pos", "zlen", "crets", "rets"):
        for off in (1, 2, 4):
            invalid(**{k: good[k] + off})
    for k in ("ccounts", "counts"):
        for off in (1, 2, 3):
            invalid(**{k: good[k] + off})
    assert call(n=0) == 0
    if no_gpu:
        assert call() == E.E_NO_DEVICE and call(mask=None) == E.E_NO_DEVICE and call(counts=None) == E.E_NO_DEVICE and call(rets=None) == E.E_NO_DEVICE
        assert call(cmask=None, ccounts=None, crets=None) == E.E_NO_DEVICE      # no chunk was decoded: nothing compact to read
        assert call(cl=5123) == E.E_NO_DEVICE


def test_tmp_bytes(lib):
    t = lib.zone_prune_tmp_bytes
    assert t(0) == 0
    for n in (1, 2, 3, 1023, 1024, 1025, 16384, 16385, 1 << 20, (1 << 20) + 1):
        b = t(n)
        assert b % 8 == 0 and b >= 4 * n + lib.compact_tmp_bytes(n)             # a flag a chunk in front of the scan's own scratch
        assert t(n + 1) >= b


# ---------------------------------------------------------------- the header's rules (zone.h on a host compiler) against the model

@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("zone") / "zone_probe"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "zone_probe.cpp"), "-o", str(exe)])

    def ask(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == len(lines), (len(out), len(lines), out[-3:])
        return [int(v) for v in out]
    return ask


def edge_values(esz):
    top = (1 << (8 * esz)) - 1
    mid = (top + 1) // 2
    return [0, 1, mid - 1, mid, top - 1, top]


def zlens(D, chunk_len):
    return [-5, 0, D - 1, D, chunk_len]


def ints(v):
    return " ".join(str(int(e)) for e in v)


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_box_rules_equal_the_model_on_the_grid(probe, esz, D):
    """lo, hi, zmin, zmax from {0, 1, mid-1, mid, top-1, top} (lo > hi and zmin > zmax among them), both modes, every zlen: D = 1 walks the
    whole grid, D = 2 and 3 a sample of theirs drawn with a fixed seed"""
    vals = edge_values(esz)
    chunk_len = 24 * D
    rng = np.random.default_rng(100 * esz + D)
    if D == 1:
        combos = [tuple((v,) for v in q) for q in itertools.product(vals, repeat=4)]
    else:
        combos = [tuple(tuple(rng.choice(vals, D)) for _ in range(4)) for _ in range(3000)]
    lines, want = [], []
    for zmin, zmax, lo, hi in combos:
        for mode in (fm.ALL, fm.ANY):
            for zlen in zlens(D, chunk_len):
                lines.append(f"box {esz} {D} {chunk_len} {zlen} 0 {mode} {ints(zmin)} {ints(zmax)} {ints(lo)} {ints(hi)}")
                want.append(zm.classify_box_chunk(zmin, zmax, zlen, lo, hi, mode, D))
    got = probe(lines)
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:5]
    assert {zm.NONE, zm.ALL, zm.DECODE} == set(want)
    # the span rule wins over everything but nothing: every chunk of a container that wide is DECODE
    wide = [" ".join(f[:5] + ["1"] + f[6:]) for f in (ln.split() for ln in lines[:200])]
    assert set(probe(wide)) == {zm.DECODE}


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_linear_rules_equal_the_model_on_the_grid(probe, esz, D):
    """test_gpu_linear.py's six weight sets without a lag term, on zones from the edge values; and forms whose bound B is 2^31 or more: where
    the zone's range leaves int32 the chunk is DECODE, where it stays inside the bounds decide"""
    vals = edge_values(esz)
    top = vals[-1]
    chunk_len = 24 * D
    rng = np.random.default_rng(200 * esz + D)
    x = rng.integers(0, top + 1, 40 * D).astype(DTYPES[esz])
    sets = [(name, [int(v) for v in w], int(bias), lo, hi) for name, w, u, bias, lo, hi in weight_sets(rng, x, esz, D, False)]
    assert len(sets) == 6 and all(lm.bound_B(esz, w, None, bias) < 1 << 31 for _, w, bias, _, _ in sets)
    big = (1 << 31) - 1
    # B >= 2^31: on the zone [top, top] the range leaves int32 (DECODE, whatever the interval), on [0, 0] it is the bias alone
    wide_forms = [("over", [big] + [0] * (D - 1), 5, None, None), ("under", [-big] + [0] * (D - 1), -5, None, None),
                  ("both", [big] * D, -(1 << 31), -7, 7)]
    assert all(lm.bound_B(esz, w, None, bias) >= 1 << 31 for _, w, bias, _, _ in wide_forms)
    lines, want, names = [], [], []
    zones = [(tuple(rng.choice(vals, D)), tuple(rng.choice(vals, D))) for _ in range(150)] + [((top,) * D, (top,) * D), ((0,) * D, (0,) * D)]
    for name, w, bias, lo, hi in sets + wide_forms:
        lo_i = lm.INT32_MIN if lo is None else int(lo)
        hi_i = lm.INT32_MAX if hi is None else int(hi)
        for zmin, zmax in zones:
            for zlen in zlens(D, chunk_len):
                lines.append(f"lin {esz} {D} {chunk_len} {zlen} 0 {bias} {lo_i} {hi_i} {ints(w)} {ints(zmin)} {ints(zmax)}")
                want.append(zm.classify_linear_chunk(zmin, zmax, zlen, w, bias, lo_i, hi_i, D))
                names.append((name, zmin, zmax, zlen))
    got = probe(lines)
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:5]
    by = {k: g for k, g in zip(names, got)}
    full = chunk_len
    assert by[("over", (top,) * D, (top,) * D, full)] == zm.DECODE               # 5 + (2^31 - 1) top > INT32_MAX
    assert by[("under", (top,) * D, (top,) * D, full)] == zm.DECODE
    assert by[("both", (top,) * D, (top,) * D, full)] == zm.DECODE
    assert by[("over", (0,) * D, (0,) * D, full)] == zm.ALL                      # the same form on a zone where it stays inside: s = 5
    assert by[("both", (0,) * D, (0,) * D, full)] == zm.NONE                     # s = -2^31, outside [-7, 7]
    assert {zm.NONE, zm.ALL, zm.DECODE} <= set(want)


def test_span_rows_and_mask_bytes(probe, lib):
    L = zm.SPAN_LIMIT
    assert probe([f"span 0 {L - 1}", f"span 0 {L}", f"span 4096 {4096 + L - 1}", f"span 4096 {4096 + L}", f"span {1 << 40} {(1 << 40) + L + 17}",
                  "span 0 0"]) == [0, 1, 0, 1, 1, 0]
    assert not zm.too_wide(0, L - 1) and zm.too_wide(0, L)
    assert probe(["rows 0 24 3", "rows 2 24 3", "rows 3 24 3", "rows 23 24 3", "rows 24 24 3", "rows 25 25 3", "rows 99 24 3"]) == [0, 0, 1, 7, 8, 8, 8]
    q, want = [], []
    for rows in (0, 1, 7, 8, 9, 15, 16, 17, 100):
        MB = -(-rows // 8) + 1
        m = zm.all_mask(rows, MB)
        for j in range(MB):
            q.append(f"byte {rows} {j}")
            want.append(int(m[j]))
    assert probe(q) == want
    for n in (1, 2, 3, 1025):
        assert probe([f"tmp {n}"])[0] + lib.compact_tmp_bytes(n) == lib.zone_prune_tmp_bytes(n)


# ---------------------------------------------------------------- soundness: what everything rests on

SHAPES = [
    # (esz, D, chunk_len, n): short last chunks, one ending mid-row, R % 8 != 0
    (1, 3, 99, 99 * 6 + 41),
    (2, 5, 80, 80 * 7 + 17),
    (1, 1, 13, 13 * 9 + 6),
    (2, 8, 8 * 21, 8 * 21 * 5 + 8 * 5 + 3),
    (1, 7, 7 * 16, 7 * 16 * 6 + 7 * 9 + 6),
    (2, 2, 64, 64 * 8),
]


def levelled(rng, n, esz, D, chunk_len):
    """chunks at random levels with a little noise: zones that are narrow and far apart, so that all three classes occur"""
    top = (1 << (8 * esz)) - 1
    nchunks = -(-n // chunk_len)
    level = rng.integers(0, top - 40, (nchunks, 1)).repeat(chunk_len, axis=1).ravel()[:n]
    return (level + rng.integers(0, 32, n)).astype(DTYPES[esz])


def chunk_rows_exist(n, chunk_len, D):
    return [ne // D for ne in fm.chunk_counts(n, chunk_len)]


def assert_sound(cls, mask, counts, rows, MB, msg):
    for c, k in enumerate(cls):
        if k == zm.NONE:
            assert not mask[c].any() and counts[c] == 0, ("NONE",) + msg + (c,)
        elif k == zm.ALL:
            assert np.array_equal(mask[c], zm.all_mask(rows[c], MB)) and counts[c] == rows[c], ("ALL",) + msg + (c,)


@pytest.mark.parametrize("esz,D,chunk_len,n", SHAPES)
def test_soundness_box(probe, esz, D, chunk_len, n):
    """the classes are zone.h's own (the probe), one query a chunk; the model must agree with them"""
    cases, lines = [], []
    rng = np.random.default_rng(esz * 1000 + D * 10 + chunk_len)
    seen = set()
    R, MB = fm.geometry(chunk_len, D)
    rows = chunk_rows_exist(n, chunk_len, D)
    top = (1 << (8 * esz)) - 1
    for trial in range(60):
        x = levelled(rng, n, esz, D, chunk_len)
        zmin, zmax, zlen = zm.zone_map(x, chunk_len, D, esz)
        c = int(rng.integers(0, len(zlen)))                          # bounds around one chunk's zone, a column or two moved
        lo, hi = zmin[c].astype(np.int64) - rng.integers(0, 3, D) * 20, zmax[c].astype(np.int64) + rng.integers(0, 3, D) * 20
        k = rng.integers(0, D)
        if trial % 3 == 1:
            lo[k] = min(top, int(zmax[c, k]) - 5)                    # ... one cuts into the zone
        if trial % 5 == 2:
            lo[k], hi[k] = 9, 3                                      # ... one never matches
        lo, hi = np.clip(lo, 0, top), np.clip(hi, 0, top)
        for mode in (fm.ALL, fm.ANY):
            lines += [f"box {esz} {D} {chunk_len} {zlen[j]} 0 {mode} {ints(zmin[j])} {ints(zmax[j])} {ints(lo)} {ints(hi)}" for j in range(len(zlen))]
            cases.append((zm.classify_box(zmin, zmax, zlen, lo, hi, mode, D), fm.filter_rows(x, chunk_len, D, lo, hi, mode), (esz, D, chunk_len, trial, mode)))
    got = probe(lines)
    for model_cls, (mask, counts), msg in cases:
        cls, got = np.array(got[:len(model_cls)], np.uint8), got[len(model_cls):]
        assert np.array_equal(cls, model_cls), ("zone.h against the model",) + msg
        assert_sound(cls, mask, counts, rows, MB, msg)
        seen |= set(int(v) for v in cls)
    assert seen == {zm.NONE, zm.ALL, zm.DECODE}


@pytest.mark.parametrize("esz,D,chunk_len,n", [s for s in SHAPES if s[2] % s[1] == 0])
def test_soundness_linear(probe, esz, D, chunk_len, n):
    """as test_soundness_box, for the linear form"""
    cases, lines = [], []
    rng = np.random.default_rng(esz * 2000 + D * 10 + chunk_len)
    seen = set()
    R, MB = fm.geometry(chunk_len, D)
    rows = chunk_rows_exist(n, chunk_len, D)
    for trial in range(40):
        x = levelled(rng, n, esz, D, chunk_len)
        zmin, zmax, zlen = zm.zone_map(x, chunk_len, D, esz)
        for name, w, u, bias, lo, hi in weight_sets(rng, x, esz, D, False):
            lo_i = lm.INT32_MIN if lo is None else int(lo)
            hi_i = lm.INT32_MAX if hi is None else int(hi)
            lines += [f"lin {esz} {D} {chunk_len} {zlen[j]} 0 {int(bias)} {lo_i} {hi_i} {ints(w)} {ints(zmin[j])} {ints(zmax[j])}" for j in range(len(zlen))]
            cases.append((zm.classify_linear(zmin, zmax, zlen, w, bias, lo, hi, D), lm.filter_linear(x, chunk_len, D, w, lo, hi, None, bias),
                          (esz, D, chunk_len, trial, name)))
    got = probe(lines)
    for model_cls, (mask, counts), msg in cases:
        cls, got = np.array(got[:len(model_cls)], np.uint8), got[len(model_cls):]
        assert np.array_equal(cls, model_cls), ("zone.h against the model",) + msg
        assert_sound(cls, mask, counts, rows, MB, msg)
        seen |= set(int(v) for v in cls)
    assert seen == {zm.NONE, zm.ALL, zm.DECODE}


# ---------------------------------------------------------------- rowops' host reference

@pytest.mark.parametrize("esz,D,chunk_len,n", SHAPES)
def test_host_reference_equals_the_model(esz, D, chunk_len, n):
    """rowops.zone_classify_* equal the model chunk for chunk (a damaged chunk and both sides of the span rule among them), and
    rowops.zone_expand, fed the unpruned model's rows of the DECODE chunks, gives back the unpruned model's mask, counts and element counts
    -- R % 8 != 0 in most of these shapes, so the ALL chunks' last mask byte has padding bits to keep clear"""
    import torch
    from sprintz_amd import rowops
    rng = np.random.default_rng(esz * 3000 + D * 10 + chunk_len)
    R, MB = fm.geometry(chunk_len, D)
    x = levelled(rng, n, esz, D, chunk_len)
    zmin, zmax, zlen = zm.zone_map(x, chunk_len, D, esz)
    zlen_d = zlen.copy()
    zlen_d[1] = -5                                                   # a chunk the zone map found damaged
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))      # noqa: E731
    seen = set()
    for c, cut in itertools.product(range(len(zlen)), (False, True)):
        lo, hi = zmin[c].astype(np.int64), zmax[c].astype(np.int64) + 3          # around chunk c's zone, or (cut) through the middle of it
        if cut:
            lo = (lo + zmax[c].astype(np.int64)) // 2
        for mode, name in ((fm.ALL, "all"), (fm.ANY, "any")):
            for span in (0, zm.SPAN_LIMIT - 1, zm.SPAN_LIMIT):
                want = zm.classify_box(zmin, zmax, zlen_d, lo, hi, mode, D, span)
                got = rowops.zone_classify_box(t(zmin), t(zmax), t(zlen_d), t(lo), t(hi), name, chunk_len, D, span).numpy()
                assert got.dtype == np.uint8 and np.array_equal(got, want), (c, name, span)
            cls = zm.classify_box(zmin, zmax, zlen, lo, hi, mode, D)
            seen |= set(int(v) for v in cls)
            mask, counts = fm.filter_rows(x, chunk_len, D, lo, hi, mode)
            dec = cls == zm.DECODE
            for expand in (zm.expand, lambda *a: tuple(v.numpy() for v in rowops.zone_expand(*[t(v) for v in a[:5]], *a[5:]))):
                m, k, r = expand(cls, zlen, mask[dec], counts[dec], zlen[dec], chunk_len, D)
                assert np.array_equal(m, mask) and np.array_equal(k, counts) and np.array_equal(r, zlen), (c, name)
    assert seen == {zm.NONE, zm.ALL, zm.DECODE}
    # a chunk the map found damaged: whatever the decoder returned for it in the survivors' container, its ret is the map's code
    cls = zm.classify_box(zmin, zmax, zlen_d, lo, hi, fm.ALL, D)
    dec = cls == zm.DECODE
    assert dec[1]
    crets = zlen[dec].copy()                                         # (the truncated chunk decoded on into its neighbour: a positive ret)
    for expand in (zm.expand, lambda *a: tuple(v.numpy() for v in rowops.zone_expand(*[t(v) for v in a[:5]], *a[5:]))):
        m, k, r = expand(cls, zlen_d, mask[dec], counts[dec], crets, chunk_len, D)
        assert np.array_equal(r, zlen_d) and r[1] == -5
    if chunk_len % D == 0:
        for name, w, u, bias, lo, hi in weight_sets(rng, x, esz, D, False):
            lo_i = lm.INT32_MIN if lo is None else int(lo)
            hi_i = lm.INT32_MAX if hi is None else int(hi)
            for span in (0, zm.SPAN_LIMIT):
                want = zm.classify_linear(zmin, zmax, zlen_d, w, bias, lo, hi, D, span)
                got = rowops.zone_classify_linear(t(zmin), t(zmax), t(zlen_d), t(w), bias, lo_i, hi_i, chunk_len, D, span).numpy()
                assert np.array_equal(got, want), (name, span)


def test_zones_of_another_layout_or_quirk_state_are_refused():
    import torch
    from sprintz_amd import ZoneMap, rowops
    z = ZoneMap(torch.zeros((4, 3), dtype=torch.uint8), torch.zeros((4, 3), dtype=torch.uint8), torch.zeros(4, dtype=torch.int64), False, 0)
    rowops.check_zones(z, 4, 3, False, 0)
    for args in ((4, 3, True, 0), (4, 3, False, 1), (5, 3, False, 0), (4, 2, False, 0)):
        with pytest.raises(ValueError):
            rowops.check_zones(z, *args)
