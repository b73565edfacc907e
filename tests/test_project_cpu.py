"""CPU tier of project rows (sprintz_mi355x_project_rows, ChunkedCodec.project_rows): the symbol and its binding are there, every validation
return comes before the device is touched, the numpy model the GPU tier compares with (tests/project_model.py) equals plain slicing, a
chunk-by-chunk evaluation and float_model on the sliced input, rowops.project_slots builds the table the model builds and refuses what it
must, and the planner (sprintz_amd/csrc/plan.h, built with g++: tests/plan_probe.cpp, asked with q=16 rows=K out_esz=...) sends the mode to
decode_fast.h exactly where the projected block is whole 16-byte pieces on a one-column-a-lane mapping."""
import os

import numpy as np
import pytest

import float_model as fm
import planner
import project_model as pm
from fixtures import buf_fixture, lib, refusals  # noqa: F401  (fixtures)
from rowdata import FLOAT_FAST_SHAPES as FAST_SHAPES, GENERIC_SHAPES, RAGGED_SHAPES

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = {1: np.uint8, 2: np.uint16}
Q_PROJECT = 16                                            # geom.h: kQueryProject


buf = buf_fixture(16384)


def test_symbol_and_binding(lib):
    assert "sprintz_mi355x_project_rows" in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.lib, "sprintz_mi355x_project_rows")
    assert len(lib.project_rows.argtypes) == 16
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_project_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    assert "uint32_t chunk_len, uint32_t ndims, const int32_t* d_slots, uint32_t ncolumns, int format," in hdr
    assert "const float* d_scale, const float* d_offset, uint32_t flags, void* d_out, int64_t* d_rets, void* hip_stream);" in hdr
    assert (lib.PROJECT_RAW, lib.PROJECT_F32, lib.PROJECT_F16, lib.PROJECT_BF16) == (0, 1 + lib.FLOAT_F32, 1 + lib.FLOAT_F16, 1 + lib.FLOAT_BF16)
    for name, v in (("SPRINTZ_PROJECT_RAW", "0"), ("SPRINTZ_PROJECT_F32", "1"), ("SPRINTZ_PROJECT_F16", "2"), ("SPRINTZ_PROJECT_BF16", "3")):
        assert f"#define {name}" in hdr and hdr.split(f"#define {name}")[1].split()[0] == v
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    geom = open(os.path.join(os.path.dirname(HERE), "sprintz_amd", "csrc", "geom.h")).read()
    assert f"kQueryProject = {Q_PROJECT};" in geom
    from sprintz_amd import ChunkedCodec
    assert callable(ChunkedCodec.project_rows)


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=8 * 67, D=8, slots=p + 1024, K=2, fmt=0, scale=None, offset=None, flags=0, out=p + 4096, rets=p + 12288)

    def call(**kw):
        a = dict(good, **kw)
        return lib.project_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["slots"], a["K"], a["fmt"], a["scale"], a["offset"],
                                a["flags"], a["out"], a["rets"], None)
    invalid, unsupported = refusals(lib, call, "project_rows")
    invalid(K=0)
    invalid(K=9)                                                                 # more output columns than the batch has
    invalid(cl=8 * 67 + 1)                                                       # chunk_len % ndims != 0
    invalid(D=7)
    invalid(cl=0)
    invalid(flags=4)                                                             # unknown flag
    invalid(flags=2)                                                             # SPRINTZ_FLOAT_SIGNED without a float format
    invalid(scale=p + 2048)                                                      # scale / offset without a float format
    invalid(offset=p + 2048)
    for fmt in (-1, 4, 7):
        invalid(fmt=fmt)
    for k in ("comp", "offs", "slots", "out"):
        invalid(**{k: None})
    invalid(out=p + 4097)                                                        # misaligned to the output element: 2 bytes raw, 4 as float32
    invalid(fmt=1, out=p + 4098)
    invalid(slots=p + 1026)
    invalid(fmt=1, scale=p + 2050)
    invalid(fmt=2, offset=p + 2049)
    invalid(rets=p + 12292)
    assert call(D=0) == E.E_INVALID and call(codec=9) == E.E_INVALID and call(esz=3) == E.E_INVALID
    unsupported(D=513, cl=513 * 64)                                              # more than 512 columns
    unsupported(D=70000, cl=70000)
    for codec in (2, 3):
        unsupported(codec=codec)                                                 # the non-RLE codecs
    assert call(n=0) == 0                                                        # nothing to do: returns 0, launches nothing
    import torch
    if not torch.cuda.is_available():
        assert call() == E.E_NO_DEVICE
        assert call(K=8) == E.E_NO_DEVICE and call(K=1, rets=None) == E.E_NO_DEVICE
        assert call(flags=1) == E.E_NO_DEVICE and call(out=p + 4098) == E.E_NO_DEVICE
        for fmt in (1, 2, 3):
            assert call(fmt=fmt, scale=p + 2048, offset=p + 3072, flags=2) == E.E_NO_DEVICE and call(fmt=fmt, flags=3) == E.E_NO_DEVICE
        assert call(fmt=2, out=p + 4098) == E.E_NO_DEVICE


# ------------------------------------------------------------------ the model

COLUMN_SETS = {
    8: [[0], [7], [1, 6], [7, 6, 5, 4, 3, 2, 1, 0], list(range(8)), [5, 0, 3], [2, 4, 6, 1]],
    5: [[0], [4], [0, 3], [4, 3, 2, 1, 0], list(range(5)), [2, 4, 1]],
    3: [[0], [2], [0, 2], [2, 1, 0], [0, 1, 2]],
    1: [[0]],
    7: [[0], [6], [1, 5], list(range(6, -1, -1)), list(range(7)), [3, 0, 6]],
}


@pytest.mark.parametrize("esz,D,chunk_len,n", RAGGED_SHAPES)
def test_model_against_slicing_and_chunks(esz, D, chunk_len, n):
    """plain numpy slicing of the batch reshaped [G, D] (zeros behind a partial last row), and the chunk-by-chunk, element-by-element walk"""
    rng = np.random.default_rng(n)
    x = rng.integers(0, 1 << (8 * esz), n).astype(DTYPES[esz])
    G = -(-n // D)
    full = np.zeros(G * D, x.dtype)
    full[:n] = x
    for cols in COLUMN_SETS[D]:
        got = pm.project(x, chunk_len, D, cols)
        assert got.dtype == x.dtype and got.shape == (G, len(cols))
        assert np.array_equal(got, full.reshape(G, D)[:, cols])
        assert np.array_equal(got, pm.project_chunks(x, chunk_len, D, cols))
        w = pm.written(n, D, cols)
        assert w.shape == got.shape and w[:n // D].all() and not got[~w].any()
        if n % D:
            assert np.array_equal(w[-1], np.array(cols) < n % D)
        assert np.array_equal(pm.slots(cols, D)[cols], np.arange(len(cols))) and (pm.slots(cols, D) >= 0).sum() == len(cols)
    if D > 1:
        assert np.array_equal(pm.project(x, chunk_len, D, range(D)).reshape(-1)[:n], x)      # the identity is the decode


@pytest.mark.parametrize("esz,D,chunk_len,n", RAGGED_SHAPES)
@pytest.mark.parametrize("fmt", fm.FORMATS)
def test_model_against_float_model(esz, D, chunk_len, n, fmt):
    """a float format: float_model applied to the sliced input with the slots' parameters, and the element-by-element walk"""
    rng = np.random.default_rng(n + fmt)
    x = rng.integers(0, 1 << (8 * esz), n).astype(DTYPES[esz])
    G = -(-n // D)
    full = np.zeros(G * D, x.dtype)
    full[:n] = x
    for cols in COLUMN_SETS[D]:
        K = len(cols)
        scale, offset = fm.column_params(K)
        for signed in (False, True):
            got = pm.project(x, chunk_len, D, cols, fmt, scale, offset, signed)
            assert got.dtype == fm.BITS_DTYPE[fmt] and got.shape == (G, K)
            # the sliced input is a batch of K columns whose every chunk is whole rows: float_model's own rule on it
            want = fm.float_rows(full.reshape(G, D)[:, cols].reshape(-1), K * (chunk_len // D), K, scale, offset, signed, fmt).reshape(G, K)
            w = pm.written(n, D, cols)
            assert np.array_equal(got[w], want[w]) and not got[~w].any()
            if G * K <= 400:
                assert np.array_equal(got, pm.project_chunks(x, chunk_len, D, cols, fmt, scale, offset, signed))
    # no parameters: scale 1, offset 0
    cols = COLUMN_SETS[D][-1]
    assert np.array_equal(pm.project(x, chunk_len, D, cols, fmt), pm.project(x, chunk_len, D, cols, fmt, np.ones(len(cols)), np.zeros(len(cols))))


# ------------------------------------------------------------------ rowops

def test_project_slots():
    import torch
    from sprintz_amd import rowops
    for D, sets in COLUMN_SETS.items():
        for cols in sets:                                                        # ascending, reversed, permuted, the identity
            for form in (cols, tuple(cols), np.array(cols), torch.tensor(cols)):
                s = rowops.project_slots(form, D)
                assert s.dtype == torch.int32 and s.shape == (D,) and np.array_equal(s.numpy(), pm.slots(cols, D))
    assert rowops.project_slots(range(4), 4).tolist() == [0, 1, 2, 3]
    assert rowops.project_slots([3, 1], 4).tolist() == [-1, 1, -1, 0]
    for bad in ([], (), [0, 0], [1, 2, 1], [8], [-1], [0, 9], [1.0], [0.5], ["0"], [None], [True], [[0]]):
        with pytest.raises(ValueError):
            rowops.project_slots(bad, 8)


# ------------------------------------------------------------------ the planner

@pytest.fixture(scope="module")
def plan():
    planner.available()
    return lambda **fields: planner.ask("decode", q=Q_PROJECT, **fields)


def named_chunk_len(D):
    return D * (16 * 4 + 3)


def out_sizes(esz):
    return sorted({esz, 2, 4})


# the named shapes at 67 rows a chunk, and one shape more for every lane mapping of decode_fast.h that those leave out (4 and 8 lanes at 8 bits, a
# partly filled group of 64): 80 rows where 67 do not make the chunk a whole number of 16-byte pieces
PLANNER_SHAPES = [(esz, D, 67) for esz, D in FAST_SHAPES + GENERIC_SHAPES] + [(2, 4, 80), (1, 6, 80), (1, 8, 80), (1, 64, 67), (2, 33, 80), (2, 40, 67), (1, 6, 67)]


@pytest.mark.parametrize("esz,D,R", PLANNER_SHAPES)
def test_planner_family(plan, esz, D, R):
    """decode_fast.h for (16 bits; 8 / 16 / 24 / 64 columns; every K) and (8 bits; 16 columns; even K); the generic kernel for odd K at 8
    bits, for the low-dim shapes, under NO_FAST, for a misaligned output and for more than 64 columns -- the two- and four-columns-a-lane
    mappings are not built for this mode, so 80, 128 and 256 columns run the generic kernel at every K"""
    chunk_len = D * R
    seen = set()
    for general in (0, 1):
        for K in sorted({1, 2, 3, 4, 5, D // 2, D - 1, D} & set(range(1, D + 1))):
            for osz in out_sizes(esz):
                for no_fast in (0, 1):
                    for cpg in (1, 3):
                        for out_lo in (0, esz):
                            got = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=5, codec=1, rows=K, out_esz=osz, general=general, no_fast=no_fast,
                                       chunks_per_group=cpg, out_lo=out_lo)
                            want = pm.fast_takes(esz, D, chunk_len, K, osz, general, no_fast, out_lo)
                            assert got.get("family") == ("dec_fast" if want else "dec_generic"), (got, K, osz, general, no_fast, out_lo)
                            if want:
                                plain = planner.ask("decode", esz=esz, D=D, chunk_len=chunk_len, nchunks=4096, codec=1, general=general, chunks_per_group=cpg)
                                assert plain["family"] == "dec_fast"             # a shape the plain decode runs there
                                assert got["cpl"] == 1 and got["dp"] == plain["dp"] and got["lds_group_stride"] == plain["lds_group_stride"], (got, plain)
                                assert got["lds"] == plain["lds"] and got["chunks_per_group"] == cpg and got["table_off"] == 0, (got, plain)
                                assert got["grid"] == -(--(-5 // cpg) * got["dp"] // 256), got
                            else:
                                assert got["lds"] == 0 and got["vec_store"] == 0 and got["grid"] == -(-5 * (1 << got["log2DP"]) // 256), got
                            if not no_fast and not out_lo:
                                seen.add((got["family"], K % 2))
    fams = {f for f, _ in seen}
    if esz == 2 and D in (4, 8, 16, 24, 33, 40, 64):
        assert fams == {"dec_fast"}                                              # every K
    elif esz == 1 and D in (6, 8, 16, 64) and (D, R) != (6, 67):                 # (6 x 67 bytes a chunk: the plain decode does not run there either)
        assert seen == {("dec_fast", 0), ("dec_generic", 1)}                     # even K alone
    else:
        assert fams == {"dec_generic"}


def test_planner_refuses_k_outside_the_row(plan):
    for esz, D in ((2, 8), (1, 16), (2, 1), (1, 80)):
        for K in (0, D + 1, 1000):
            got = plan(esz=esz, D=D, chunk_len=named_chunk_len(D), nchunks=5, codec=0, rows=K, out_esz=esz)
            assert got.get("error") == -1 and "project_rows" in got["what"], got      # SPRINTZ_E_INVALID
    for codec in (2, 3):
        assert plan(esz=1, D=8, chunk_len=8 * 67, nchunks=5, codec=codec, rows=2, out_esz=1).get("error") == -4


def test_planner_reach_counts_projected_bytes(plan):
    """the wave's chunks lie within 32-bit offsets of its first: 4096 projected slots below 0xf0000000 bytes -- both sides of the edge at uint16 x 8
    to float32, where two columns stay inside and all eight do not"""
    D, R = 8, 100000
    assert R * 2 * 4 * 4096 < 0xf0000000 <= R * 3 * 4 * 4096
    for K, fam in ((1, "dec_fast"), (2, "dec_fast"), (3, "dec_generic"), (8, "dec_generic")):
        assert plan(esz=2, D=D, chunk_len=D * R, nchunks=5, codec=1, rows=K, out_esz=4)["family"] == fam
    assert plan(esz=2, D=D, chunk_len=D * R, nchunks=5, codec=1, rows=8, out_esz=2)["family"] == "dec_generic"
    assert plan(esz=2, D=D, chunk_len=D * R, nchunks=5, codec=1, rows=4, out_esz=2)["family"] == "dec_fast"


def test_planner_leaves_the_other_modes_alone():
    """rows and out_esz mean nothing to the plain decode: its plan is the one it had"""
    planner.available()
    base = dict(esz=2, D=8, chunk_len=5120, nchunks=4096, codec=1)
    assert planner.ask("decode", **base) == planner.ask("decode", rows=2, **base)
    assert planner.ask("decode", **base)["family"] == "dec_fast"
