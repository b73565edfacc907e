"""CPU tier of float rows (sprintz_mi355x_float_rows, ChunkedCodec.float_rows): the symbol and its binding are there, every validation
return comes before the device is touched, the numpy model the GPU tier compares with (tests/float_model.py) equals torch's
(x.to(float32) * scale + offset).to(dtype) on the CPU bit for bit and a one-element-at-a-time brute force, the planner
(sprintz_amd/csrc/plan.h, built with g++: tests/plan_probe.cpp) sends the mode to decode_fast.h or to the generic kernel where the
header says, and datasets.dequantize_params inverts datasets.quantize within one step."""
import os

import numpy as np
import pytest

import float_model as fm
from fixtures import buf_fixture, lib  # noqa: F401  (fixtures)
from planner import QUERY, plan_fixture
from rowdata import FLOAT_FAST_SHAPES as FAST_SHAPES, GENERIC_SHAPES, RAGGED_SHAPES as SHAPES

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = {1: np.uint8, 2: np.uint16}


buf = buf_fixture(8192)


def test_symbol_and_binding(lib):
    assert "sprintz_mi355x_float_rows" in lib.EXPORTED_SYMBOLS
    assert hasattr(lib.lib, "sprintz_mi355x_float_rows")
    assert len(lib.float_rows.argtypes) == 14
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_float_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    assert "uint32_t chunk_len, uint16_t ndims, int out_format, const float* d_scale, const float* d_offset," in hdr
    assert (lib.FLOAT_F32, lib.FLOAT_F16, lib.FLOAT_BF16, lib.FLOAT_SIGNED) == (0, 1, 2, 2)
    for name, v in (("SPRINTZ_FLOAT_F32", "0"), ("SPRINTZ_FLOAT_F16", "1"), ("SPRINTZ_FLOAT_BF16", "2"), ("SPRINTZ_FLOAT_SIGNED", "2u")):
        assert f"#define {name}" in hdr and hdr.split(f"#define {name}")[1].split()[0] == v
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    from sprintz_amd import ChunkedCodec, datasets
    assert callable(ChunkedCodec.float_rows) and callable(datasets.dequantize_params)


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    good = dict(codec=1, esz=2, comp=p, offs=p, n=3, cl=5120, D=8, fmt=0, scale=p + 128, offset=p + 256, flags=0, out=p + 2048, rets=p + 6144)

    def call(**kw):
        a = dict(good, **kw)
        return lib.float_rows(a["codec"], a["esz"], a["comp"], a["offs"], a["n"], a["cl"], a["D"], a["fmt"], a["scale"], a["offset"],
                              a["flags"], a["out"], a["rets"], None)

    assert call(cl=5121) == E.E_INVALID and call(cl=5120, D=7) == E.E_INVALID   # chunk_len % ndims != 0
    assert "float_rows" in lib.last_error()
    assert call(cl=0) == E.E_INVALID and call(cl=(1 << 30) + 8) == E.E_INVALID   # chunk_len outside 1..2^30
    assert "float_rows" in lib.last_error()
    assert call(flags=4) == E.E_INVALID and call(flags=7) == E.E_INVALID         # unknown flag (GENERAL_LAYOUT = 1 and FLOAT_SIGNED = 2 are known)
    assert "float_rows" in lib.last_error()
    assert call(fmt=3) == E.E_INVALID and call(fmt=-1) == E.E_INVALID            # unknown out_format
    assert "float_rows" in lib.last_error()
    for k in ("comp", "offs", "out"):
        assert call(**{k: None}) == E.E_INVALID, k                               # NULL pointers
        assert "float_rows" in lib.last_error()
    # d_out misaligned for each format: float32 needs 4 bytes, the 16-bit formats 2
    assert call(fmt=0, out=p + 2049) == E.E_INVALID and call(fmt=0, out=p + 2050) == E.E_INVALID
    assert call(fmt=1, out=p + 2049) == E.E_INVALID and call(fmt=2, out=p + 2049) == E.E_INVALID
    assert "float_rows" in lib.last_error()
    assert call(rets=p + 6148) == E.E_INVALID                                    # d_rets off 8 bytes
    assert call(scale=p + 130) == E.E_INVALID and call(offset=p + 257) == E.E_INVALID
    assert call(D=0) == E.E_INVALID and call(codec=9) == E.E_INVALID and call(esz=3) == E.E_INVALID
    assert call(D=513, cl=513 * 16) == E.E_UNSUPPORTED                           # more than 512 columns
    assert "float_rows" in lib.last_error()
    for codec in (2, 3):
        assert call(codec=codec) == E.E_UNSUPPORTED                              # the non-RLE codecs
    assert call(codec=4, esz=1) == E.E_UNSUPPORTED
    assert "float_rows" in lib.last_error()
    assert call(n=0) == 0                                                        # nothing to do: returns 0, launches nothing
    import torch
    if not torch.cuda.is_available():
        assert call() == E.E_NO_DEVICE
        assert call(scale=None) == E.E_NO_DEVICE and call(offset=None) == E.E_NO_DEVICE and call(rets=None) == E.E_NO_DEVICE
        assert call(scale=None, offset=None, rets=None) == E.E_NO_DEVICE
        for fmt in (0, 1, 2):
            for flags in (0, 1, 2, 3):
                assert call(fmt=fmt, flags=flags) == E.E_NO_DEVICE
        assert call(fmt=1, out=p + 2050) == E.E_NO_DEVICE and call(fmt=0, out=p + 2052) == E.E_NO_DEVICE   # off the 16-byte grid: the generic kernel's
        assert call(flags=1, D=512, cl=512 * 16) == E.E_NO_DEVICE


# ------------------------------------------------------------------ the model

def torch_bits(x, scale, offset, signed, fmt):
    """(x.to(float32) * scale + offset).to(dtype) of torch on the CPU, as bits"""
    import torch
    esz = x.dtype.itemsize
    xs = torch.from_numpy(x.view(np.int8 if esz == 1 else np.int16).copy())
    v = xs.to(torch.float32) if signed else (xs.to(torch.int32) & ((1 << (8 * esz)) - 1)).to(torch.float32)
    z = v * torch.tensor(scale, dtype=torch.float32) + torch.tensor(offset, dtype=torch.float32)
    if fmt == fm.F32:
        return z.view(torch.int32).numpy().view(np.uint32)
    return z.to(torch.float16 if fmt == fm.F16 else torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("signed", [False, True])
def test_model_equals_torch_on_the_cpu(esz, signed):
    """every value of the element type, three formats, the eight parameter pairs: bit for bit -- results that overflow to inf, float32
    subnormals and bfloat16 ties among them"""
    x = np.arange(1 << (8 * esz), dtype=np.uint32).astype(DTYPES[esz])
    seen_inf = seen_sub = seen_tie = False
    for s, o in fm.PAIRS:
        z = fm.affine(fm.values(x, signed), np.float32(s), np.float32(o))
        seen_inf |= bool(np.isinf(z).any())
        seen_sub |= bool(((np.abs(z) < 2.0 ** -126) & (z != 0)).any())
        seen_tie |= bool(((z.view(np.uint32) & 0xFFFF) == 0x8000).any())
        assert not np.isnan(z).any()                                               # finite parameters: no NaN
        for fmt in fm.FORMATS:
            got, want = fm.convert(x, np.float32(s), np.float32(o), signed, fmt), torch_bits(x, s, o, signed, fmt)
            assert got.dtype == want.dtype and np.array_equal(got, want), (esz, signed, s, o, fm.NAMES[fmt], int((got != want).sum()))
    assert seen_inf and seen_sub and (seen_tie or esz == 1)


def test_the_definition_on_cases_by_hand():
    x = np.array([0, 1, 255, 128], np.uint8)
    assert fm.convert(x, 1.0, 0.0, False, fm.F32).view(np.float32).tolist() == [0.0, 1.0, 255.0, 128.0]
    assert fm.convert(x, 1.0, 0.0, True, fm.F32).view(np.float32).tolist() == [0.0, 1.0, -1.0, -128.0]
    assert fm.convert(x, 0.5, -3.0, False, fm.F16).view(np.float16).tolist() == [-3.0, -2.5, 124.5, 61.0]
    # bfloat16 keeps 8 significant bits: 257 = 0x101 is a tie between 256 and 258 -> even (256); 259 -> 260 (0x4382)
    y = np.array([257, 259, 65535], np.uint16)
    assert fm.convert(y, 1.0, 0.0, False, fm.BF16).tolist() == [0x4380, 0x4382, 0x4780]
    assert fm.convert(y, 1.0, 0.0, False, fm.F16).view(np.float16).tolist()[:2] == [257.0, 259.0]
    assert fm.convert(y, 3e38, 1.0, False, fm.F32).tolist() == [0x7F800000] * 3   # overflow: +inf
    # two roundings, not one fma: 3 * (1 + 2^-23) = 3 + 1.5 ulp is a tie that rounds to even, 3 + 2 ulp = 3 + 2^-21, so the sum with -3 is
    # 2^-21; fused, it would be 3 * 2^-23
    s = np.float32(1 + 2.0 ** -23)
    assert fm.convert(np.array([3], np.uint8), s, -3.0, False, fm.F32).view(np.float32)[0] == np.float32(2.0 ** -21)


@pytest.mark.parametrize("esz,D,chunk_len,n", SHAPES)
def test_model_equals_brute_force(esz, D, chunk_len, n):
    """column assignment over chunks: short last chunks, one ending mid-row"""
    rng = np.random.default_rng(esz * 1000 + D)
    x = rng.integers(0, 1 << (8 * esz), n).astype(DTYPES[esz])
    scale, offset = fm.column_params(D)
    for signed in (False, True):
        for fmt in fm.FORMATS:
            assert np.array_equal(fm.float_rows(x, chunk_len, D, scale, offset, signed, fmt), fm.float_rows_brute(x, chunk_len, D, scale, offset, signed, fmt))
    ident = fm.float_rows(x, chunk_len, D)
    assert np.array_equal(ident.view(np.float32), x.astype(np.float32))
    assert np.array_equal(ident, fm.float_rows(x, chunk_len, D, np.ones(D), np.zeros(D)))


# ------------------------------------------------------------------ the planner

plan = plan_fixture(codec=1, nchunks=4096, q=QUERY["float"], out_esz=4)


def rows16(D, esz=2):
    """a chunk of whole groups of 16 rows: about 10 KB, and at least four groups (decode_fast.h takes no chunk much shorter than its
    read-ahead ring)"""
    return D * 16 * max(4, 10240 // (16 * D * esz))


def test_planner_sends_the_mode_to_decode_fast_or_the_generic_kernel(plan):
    families = set()
    for esz, D in FAST_SHAPES:
        for out_esz in (4, 2):
            for nchunks in (5, 4096, 131072):                                    # (small batches too: no workgroup-per-chunk kernel takes the mode)
                for codec in (0, 1):
                    got = plan(esz=esz, D=D, chunk_len=rows16(D, esz), out_esz=out_esz, nchunks=nchunks, codec=codec)
                    assert got["family"] == "dec_fast", (esz, D, out_esz, nchunks, got)
                    families.add(got["family"])
            # the output off by one element, OPT_NO_FAST: the generic kernel, which stages nothing
            for kw in (dict(out_lo=out_esz), dict(no_fast=1)):
                got = plan(esz=esz, D=D, chunk_len=rows16(D, esz), out_esz=out_esz, **kw)
                assert got["family"] == "dec_generic" and got["lds"] == 0 and got["vec_store"] == 0, (esz, D, out_esz, kw, got)
    head = plan(esz=2, D=8, chunk_len=5120, out_esz=2, nchunks=131072)
    assert head["family"] == "dec_fast" and head["dp"] == 8 and head["cpl"] == 1 and head["exact"] == 1
    for esz, D in GENERIC_SHAPES:
        for general in (0, 1):
            for out_esz in (4, 2):
                got = plan(esz=esz, D=D, chunk_len=rows16(D, esz), out_esz=out_esz, general=general)
                assert got["family"] == "dec_generic" and got["lds"] == 0, (esz, D, general, got)   # decode_uni.h is not taught the mode
                families.add(got["family"])
    assert families == {"dec_fast", "dec_generic"}


def test_planner_counts_the_reach_in_output_bytes(plan):
    """chunk_len * out_bytes * 4096 must stay below 0xf0000000: a chunk length at which the input's bytes pass and the output's do not"""
    limit = 0xF0000000
    for esz, D, out_esz in ((1, 16, 4), (1, 16, 2), (2, 8, 4)):
        cl = ((limit - 1) // (out_esz * 4096)) // (16 * D) * (16 * D)                 # the largest whole-group chunk that still fits
        assert cl * out_esz * 4096 < limit
        assert plan(esz=esz, D=D, chunk_len=cl, out_esz=out_esz, nchunks=64)["family"] == "dec_fast"
        cl += 16 * D
        assert cl * out_esz * 4096 >= limit and cl * esz * 4096 < limit
        assert plan(esz=esz, D=D, chunk_len=cl, out_esz=out_esz, nchunks=64)["family"] == "dec_generic"
    # uint16 -> 16-bit floats: the output's bytes are the input's, and the plain decode's bound holds
    cl = ((limit - 1) // (2 * 4096)) // 128 * 128
    assert plan(esz=2, D=8, chunk_len=cl, out_esz=2, nchunks=64)["family"] == "dec_fast"
    assert plan(esz=2, D=8, chunk_len=cl + 128, out_esz=2, nchunks=64)["family"] == "dec_generic"


# ------------------------------------------------------------------ dequantize_params

@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_dequantize_params_inverts_quantize_within_one_step(dtype):
    from sprintz_amd import datasets
    rng = np.random.default_rng(11)
    top = 255 if dtype == np.uint8 else 65535
    for rows, cols in ((200, 5), (64, 1), (1000, 8)):
        m = rng.normal(size=(rows, cols)) * rng.uniform(0.01, 1000.0, size=cols) + rng.uniform(-500, 500, size=cols)
        m[:, 0] = 3.25                                                             # a constant column
        if cols > 2:
            m[:, 2] = np.round(m[:, 2])                                            # integers
        q = datasets.quantize(m, dtype)
        scale, offset = datasets.dequantize_params(m, dtype)
        assert scale.dtype == np.float32 and offset.dtype == np.float32 and scale.shape == (cols,) and offset.shape == (cols,)
        assert np.all(np.isfinite(scale)) and np.all(scale > 0)
        span = m.max(axis=0) - m.min(axis=0)
        assert np.allclose(scale, np.maximum(1, span) / top, rtol=1e-6) and np.allclose(offset, m.min(axis=0), rtol=1e-6, atol=1e-30)
        back = fm.float_rows(q.reshape(-1), q.size, cols, scale, offset).view(np.float32).reshape(rows, cols)
        # quantize truncates (m - min) / max(1, span) * top in float32 arithmetic: the reconstruction lies at most one step (scale) below the value,
        # plus the float32 roundings of quantize's three operations and the model's two -- each at most 2^-24 of the largest magnitude about
        slack = 8 * 2.0 ** -24 * (np.abs(m).max(axis=0) + np.maximum(1, span))
        err = back.astype(np.float64) - m
        assert np.all(err <= slack) and np.all(err >= -(scale.astype(np.float64) + slack)), (dtype, rows, cols, err.min(axis=0), err.max(axis=0), scale)
    with pytest.raises(ValueError):
        datasets.dequantize_params(m, np.int32)


def test_python_side_refusals():
    """ChunkedCodec.float_rows' host checks need no device: the dtype, and host parameters that are not finite or not ndims long"""
    import torch
    from sprintz_amd import rowops
    assert [rowops.float_format(d) for d in (torch.float32, torch.float16, torch.bfloat16)] == [0, 1, 2]
    for bad in (torch.float64, torch.int16, None):
        with pytest.raises(ValueError):
            rowops.float_format(bad)
    dev = torch.device("cpu")
    assert rowops.float_params(None, 4, "scale", dev) is None
    assert rowops.float_params(0.5, 3, "scale", dev).tolist() == [0.5, 0.5, 0.5]
    t = rowops.float_params([1, 2, 3], 3, "offset", dev)
    assert t.dtype == torch.float32 and t.is_contiguous() and t.tolist() == [1.0, 2.0, 3.0]
    assert rowops.float_params(torch.arange(3, dtype=torch.float64), 3, "scale", dev).dtype == torch.float32
    for bad in (float("inf"), float("nan"), [1.0, float("-inf")], 1e39):
        with pytest.raises(ValueError):
            rowops.float_params(bad, 2, "scale", dev)
    for bad in ([1.0, 2.0, 3.0], torch.ones(5)):
        with pytest.raises(ValueError):
            rowops.float_params(bad, 2, "offset", dev)
