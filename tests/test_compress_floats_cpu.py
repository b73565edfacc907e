"""CPU tier of compress floats (sprintz_mi355x_compress_batch_float / _float_dense, ChunkedCodec.compress_floats): the symbols and their
bindings are there, every validation return comes before the device is touched and names the call, the numpy model the GPU tier compares
with (tests/quant_model.py) equals torch's nan_to_num(round_or_floor((x.float() - offset) * inv_scale), nan=0).clamp(LO, HI) on the CPU bit
for bit -- over every float16 and every bfloat16 pattern and a crafted float32 set -- and a one-element-at-a-time brute force, the planner
(sprintz_amd/csrc/plan.h through tests/plan_probe.cpp) sends a float source to encode_wide.h's kernels or the generic one and to nothing
else, and rowops.quant_params is numpy's float32 reciprocal."""
import os

import numpy as np
import pytest

import planner
import quant_model as qm
from fixtures import buf_fixture, lib  # noqa: F401  (fixtures)
from rowdata import NDIMS, RAGGED_SHAPES

HERE = os.path.dirname(os.path.abspath(__file__))
FLOAT = planner.QUERY["float"]

buf = buf_fixture(16384)


# ------------------------------------------------------------------ the bindings

def test_symbols_and_bindings(lib):
    for name in ("sprintz_mi355x_compress_batch_float", "sprintz_mi355x_compress_batch_float_dense"):
        assert name in lib.EXPORTED_SYMBOLS and hasattr(lib.lib, name)
    assert len(lib.compress_batch_float.argtypes) == 15 and len(lib.compress_batch_float_dense.argtypes) == 18
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_compress_batch_float(int codec, int elem_bytes, const void* d_src, int src_format, const float* d_inv_scale," in hdr
    assert "int sprintz_mi355x_compress_batch_float_dense(int codec, int elem_bytes, const void* d_src, int src_format, const float* d_inv_scale," in hdr
    assert "uint64_t* d_offsets, void* d_tmp, void* hip_stream);" in hdr
    assert (lib.FLOAT_F32, lib.FLOAT_F16, lib.FLOAT_BF16, lib.FLOAT_SIGNED, lib.QUANT_FLOOR) == (0, 1, 2, 2, 4)
    for name, v in (("SPRINTZ_FLOAT_F32", "0"), ("SPRINTZ_FLOAT_F16", "1"), ("SPRINTZ_FLOAT_BF16", "2"), ("SPRINTZ_FLOAT_SIGNED", "2u"), ("SPRINTZ_QUANT_FLOOR", "4u")):
        assert f"#define {name}" in hdr and hdr.split(f"#define {name}")[1].split()[0] == v
    assert "compress_batch_float / compress_batch_float_dense, SPRINTZ_QUANT_FLOOR" in hdr            # the "later, additively" line
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    assert "#define SPRINTZ_MI355X_ABI_VERSION 7" in hdr and "#define SPRINTZ_KF_COUNT" in hdr and hdr.split("#define SPRINTZ_KF_COUNT")[1].split()[0] == "33"
    from sprintz_amd import ChunkedCodec, rowops
    assert callable(ChunkedCodec.compress_floats) and callable(rowops.quant_params)


# ------------------------------------------------------------------ validation

@pytest.mark.parametrize("dense", [False, True])
def test_validation_comes_before_the_device(lib, buf, dense):
    _, p = buf
    E = lib
    name = "compress_batch_float_dense" if dense else "compress_batch_float"
    stride = int(lib.compress_bound(2, 5120, 8))
    good = dict(codec=1, esz=2, src=p, fmt=0, inv=p + 128, off=p + 256, flags=0, total=3 * 5120, cl=5120, D=8, slots=p + 512, stride=stride,
                sizes=p + 1024, rets=p + 2048, dense=p + 4096, offsets=p + 8192, tmp=p + 12288)

    def call(**kw):
        a = dict(good, **kw)
        if "stride" not in kw and a["esz"] in (1, 2) and a["D"]:
            a["stride"] = int(lib.compress_bound(a["esz"], a["cl"], a["D"]))
        head = (a["codec"], a["esz"], a["src"], a["fmt"], a["inv"], a["off"], a["flags"], a["total"], a["cl"], a["D"], a["slots"], a["stride"], a["sizes"], a["rets"])
        if dense:
            return lib.compress_batch_float_dense(*head, a["dense"], a["offsets"], a["tmp"], None)
        return lib.compress_batch_float(*head, None)

    def refused(code, **kw):
        got = call(**kw)
        assert got == code, (name, kw, got)
        err = lib.last_error()
        assert err.startswith(name + ":"), (name, kw, err)

    refused(E.E_INVALID, cl=5121)                                              # chunk_len % ndims != 0
    refused(E.E_INVALID, D=7)
    refused(E.E_INVALID, cl=0)                                                 # chunk_len outside 1..2^30
    refused(E.E_INVALID, cl=(1 << 30) + 8, stride=1 << 20)
    for fmt in (3, -1, 7):
        refused(E.E_INVALID, fmt=fmt)                                          # unknown format
    for flags in (1, 8, 16, 7, 1 << 31):
        refused(E.E_INVALID, flags=flags)                                      # unknown flag (FLOAT_SIGNED = 2 and QUANT_FLOOR = 4 are known)
    for k in ("src", "slots", "sizes") + (("dense", "offsets", "tmp") if dense else ()):
        refused(E.E_INVALID, **{k: None})                                      # NULL pointers
    refused(E.E_INVALID, fmt=0, src=p + 2)                                     # d_src off the source element: float32 needs 4 bytes ...
    refused(E.E_INVALID, fmt=0, src=p + 1)
    refused(E.E_INVALID, fmt=1, src=p + 1)                                     # ... the 16-bit formats 2
    refused(E.E_INVALID, fmt=2, src=p + 3)
    refused(E.E_INVALID, inv=p + 130)                                          # parameters off 4 bytes
    refused(E.E_INVALID, off=p + 257)
    refused(E.E_INVALID, slots=p + 516)                                        # what check_slots refuses
    refused(E.E_INVALID, stride=stride + 8)
    refused(E.E_INVALID, stride=stride - 16)
    if dense:
        refused(E.E_INVALID, dense=p + 4100)
        refused(E.E_INVALID, tmp=p + 12292)
    refused(E.E_INVALID, D=0)                                                  # what every batched call refuses
    refused(E.E_INVALID, codec=9)
    refused(E.E_INVALID, esz=3, stride=stride)
    refused(E.E_UNSUPPORTED, D=513, cl=513 * 16)                               # more than 512 columns
    for codec in (2, 3):
        refused(E.E_UNSUPPORTED, codec=codec)                                  # the non-RLE codecs
    refused(E.E_UNSUPPORTED, codec=4, esz=1)
    refused(E.E_UNSUPPORTED, D=4096, cl=4096 * 32)                             # (before check_batch_tail's own refusal: more than 512 columns)
    assert call(total=0) == 0                                                  # nothing to do: returns 0, launches nothing
    import torch
    if not torch.cuda.is_available():
        def no_device(**kw):
            assert call(**kw) == E.E_NO_DEVICE, kw
            assert lib.last_error().startswith(name + ":")
        no_device()
        no_device(inv=None)
        no_device(off=None)
        no_device(inv=None, off=None, rets=None)
        for fmt in (0, 1, 2):
            for flags in (0, 2, 4, 6):
                no_device(fmt=fmt, flags=flags)
        no_device(fmt=0, src=p + 4)                                            # off the 16-byte grid: the generic kernel's
        no_device(fmt=1, src=p + 2)
        no_device(esz=1, D=512, cl=512 * 16)
        no_device(total=3 * 5120 - 37)                                         # a short last chunk that ends mid-row


# ------------------------------------------------------------------ the model

def torch_quantize(v, inv, off, W, signed, floor):
    """nan_to_num(round_or_floor((x.float() - offset) * inv_scale), nan=0).clamp(LO, HI) of torch on the CPU -> the W-bit elements"""
    import torch
    lo, hi = qm.limits(W, signed)
    x = torch.from_numpy(np.ascontiguousarray(v, np.float32))
    t = (x.float() - torch.tensor(off, dtype=torch.float32)) * torch.tensor(inv, dtype=torch.float32)
    r = torch.floor(t) if floor else torch.round(t)
    q = torch.nan_to_num(r, nan=0.0).clamp(lo, hi).to(torch.int64).numpy()
    return (q & ((1 << W) - 1)).astype(qm.DTYPES[W])


def torch_source(bits, fmt):
    """the 16-bit patterns as torch reads them -> float32 values"""
    import torch
    t = torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16 if fmt == qm.F16 else torch.bfloat16)
    return t.float().numpy()


def crafted_float32(W, signed, inv, off):
    """exact ties k + 0.5 in q's terms, both clamp ends and one step past them, -0.0, subnormals, +-inf, NaN, 3e38 -- as x with
    (x - off) * inv near the wanted t, and the same as plain values"""
    lo, hi = qm.limits(W, signed)
    t = np.array([lo - 1.5, lo - 1, lo - 0.5, lo, lo + 0.5, lo + 1.5, -2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5, hi - 1.5, hi - 0.5, hi, hi + 0.5, hi + 1, hi + 1.5, 1e6, -1e6],
                 np.float64)
    with np.errstate(all="ignore"):
        x = (t / np.float64(inv) + np.float64(off)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, 2.0 ** -126, np.inf, -np.inf, np.nan, 3e38, -3e38, 0.5, 1.5, 2.5, -0.5, 254.5, 255.5, 65534.5, 65535.5,
                        127.5, -128.5, 32767.5, -32768.5], np.float32)
    return np.concatenate([x, t.astype(np.float32), special])


@pytest.mark.parametrize("W", [8, 16])
@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("floor", [False, True])
def test_model_equals_torch_on_the_cpu(W, signed, floor):
    """every float16 pattern, every bfloat16 pattern and the crafted float32 set, under the eight parameter pairs: bit for bit"""
    lo, hi = qm.limits(W, signed)
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    seen = dict(nan=False, inf=False, tie=False, lo=False, hi=False)
    for inv, off in qm.PAIRS:
        sources = [(qm.NAMES[fmt], qm.source_values(bits, fmt), torch_source(bits, fmt)) for fmt in (qm.F16, qm.BF16)]
        c = crafted_float32(W, signed, inv, off)
        sources.append(("float32", c, c))
        for name, v, tv in sources:
            assert np.array_equal(v.view(np.uint32), tv.view(np.uint32)) or np.array_equal(np.isnan(v), np.isnan(tv)), name     # the source reads the same
            got, want = qm.quantize(v, np.float32(inv), np.float32(off), W, signed, floor), torch_quantize(tv, inv, off, W, signed, floor)
            assert got.dtype == want.dtype and np.array_equal(got, want), (W, signed, floor, inv, off, name, int((got != want).sum()),
                                                                            v[np.flatnonzero(got != want)[:4]].tolist())
            with np.errstate(all="ignore"):
                t = ((v - np.float32(off)).astype(np.float32) * np.float32(inv)).astype(np.float32)
            seen["nan"] |= bool(np.isnan(t).any())
            seen["inf"] |= bool(np.isinf(t).any())
            fin = t[np.isfinite(t)]
            seen["tie"] |= bool(((np.abs(fin) < 2.0 ** 22) & (fin - np.floor(fin) == 0.5)).any())
            seen["lo"] |= bool((fin < lo).any())
            seen["hi"] |= bool((fin > hi).any())
    assert all(seen.values()), seen


def test_the_definition_on_cases_by_hand():
    f = np.float32
    q8 = lambda v, **kw: qm.quantize(np.array(v, np.float32), f(1), f(0), 8, **kw).tolist()      # noqa: E731
    assert q8([0.5, 1.5, 2.5, 3.5, -0.5, 254.5, 255.5, 300.0, -3.0]) == [0, 2, 2, 4, 0, 254, 255, 255, 0]        # ties to even; both clamp ends
    assert q8([0.5, 1.5, 2.5, -0.5, 255.9], floor=True) == [0, 1, 2, 0, 255]
    assert q8([np.nan, np.inf, -np.inf, -0.0, 3e38]) == [0, 255, 0, 0, 255]
    assert q8([np.nan, np.inf, -np.inf], signed=True) == [0, 127, 128]
    assert q8([-1.0, -128.5, -129.0, 127.4, 127.5, 200.0], signed=True) == [255, 128, 128, 127, 127, 127]        # two's complement; 127.5 -> 128 -> clamped
    q16 = qm.quantize(np.array([65534.5, 65535.5, -32768.5, 40000.0], np.float32), f(1), f(0), 16, signed=True).tolist()
    assert q16 == [32767, 32767, 32768, 32767]
    # two operations, not one fused: (3 - 1) * 0.5 and the offset first
    assert qm.quantize(np.array([3.0], np.float32), f(0.5), f(1.0), 8).tolist() == [1]
    # the subtraction rounds on its own: 2^24 + 1 is not a float32, (2^24 + 2) - 1 rounds to 2^24 (ties to even)
    assert qm.quantize(np.array([2.0 ** 24 + 2], np.float32), f(2.0 ** -17), f(1.0), 8).tolist() == [128]
    # bfloat16 and float16 sources are exact in float32
    assert qm.source_values(qm.source_bits([1.0, -2.5, 65504.0], qm.F16), qm.F16).tolist() == [1.0, -2.5, 65504.0]
    assert qm.source_values(qm.source_bits([1.0, 257.0, 259.0, -0.0], qm.BF16), qm.BF16).tolist() == [1.0, 256.0, 260.0, -0.0]      # (ties to even)


@pytest.mark.parametrize("esz,D,chunk_len,n", RAGGED_SHAPES)
def test_model_equals_brute_force(esz, D, chunk_len, n):
    """column assignment over chunks -- short last chunks, one ending mid-row -- and the arithmetic, one element at a time"""
    rng = np.random.default_rng(esz * 1000 + D)
    W = 8 * esz
    inv, off = qm.column_params(D)
    with np.errstate(all="ignore"):
        v = (rng.integers(-40, (1 << W) + 40, n) + rng.choice([0.0, 0.5, 0.25, -0.5, 0.49], n)).astype(np.float64)
        d = (np.arange(n) % chunk_len) % D
        x = (v / inv[d].astype(np.float64) + off[d].astype(np.float64)).astype(np.float32)
    x[::17] = np.nan
    x[5::29] = np.inf
    x[7::31] = -np.inf
    for signed in (False, True):
        for floor in (False, True):
            got = qm.compress_floats(x, chunk_len, D, W, inv, off, signed, floor)
            want = [qm.quantize_one(x[i], inv[d[i]], off[d[i]], W, signed, floor) for i in range(n)]
            assert got.tolist() == want, (esz, D, signed, floor)
    ident = qm.compress_floats(np.arange(n, dtype=np.float32) % (1 << W), chunk_len, D, W)
    assert np.array_equal(ident, (np.arange(n) % (1 << W)).astype(qm.DTYPES[W]))


# ------------------------------------------------------------------ the planner

def rows16(D, esz):
    """a chunk of whole groups of 16 rows, about 10 KB, and at least four groups"""
    return D * 16 * max(4, 10240 // (16 * D * esz))


def shape(esz, D, chunk_len=None, nchunks=4096, **kw):
    chunk_len = rows16(D, esz) if chunk_len is None else chunk_len
    return dict(dict(codec=1, esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, total_len=nchunks * chunk_len, slot_stride=planner.bound(esz, chunk_len, D)), **kw)


NAMED = [((2, 8), "enc_pair"), ((2, 5), "enc_pair"), ((1, 16), "enc_pair"), ((2, 128), "enc_wide"), ((1, 80), "enc_split"), ((1, 128), "enc_wide"),
         ((2, 1), "enc_generic"), ((2, 2), "enc_generic"), ((2, 3), "enc_generic"), ((1, 4), "enc_generic"), ((1, 7), "enc_generic")]
EXCLUDED = {"enc_lat", "enc_blk", "enc_blk_uni", "enc_uni", "enc_fast", "enc_any", "enc_big"}


def test_planner_sends_a_float_source_to_the_kernels_that_quantise():
    planner.available()
    for (esz, D), family in NAMED:
        for out_esz in (4, 2):
            for nchunks in (1, 5, 4096, 131072):                                   # (small batches too: the enc_pair threshold does not count)
                for pair in (0, 1, 1024):
                    got = planner.ask("encode", q=FLOAT, out_esz=out_esz, enc_pair=pair, **shape(esz, D, nchunks=nchunks))
                    assert got["family"] == family, (esz, D, out_esz, nchunks, pair, got)
            got = planner.ask("encode", q=FLOAT, out_esz=out_esz, no_fast=1, **shape(esz, D))
            assert got["family"] == "enc_generic", (esz, D, got)                   # no_fast still forces the generic kernel
            got = planner.ask("encode", q=FLOAT, out_esz=out_esz, src_lo=4, **shape(esz, D))
            assert got["family"] == "enc_generic", (esz, D, got)                   # a source off the 16-byte grid
    # the headline shape: the container inside the launch
    head = planner.ask("encode", q=FLOAT, out_esz=4, dense=1, **shape(2, 8, 5120, 192))
    assert head["family"] == "enc_pair" and head["fused"] == 1 and head["dp"] == 4 and head["exact"] == 1
    assert planner.ask("dense", q=FLOAT, out_esz=4, **shape(2, 8, 5120, 192)) == {"family": "dense_fused", "enc": "enc_pair"}
    # the parameter table of encode_wide.h's kernels rides behind the groups' carves: 64 D bytes more than the integer plan
    for esz, D in ((2, 8), (1, 80), (2, 128)):
        f, i = planner.ask("encode", q=FLOAT, out_esz=4, **shape(esz, D)), planner.ask("encode", enc_pair=1, lat_chunks=0, blk_chunks=0, **shape(esz, D))
        assert f["family"] == i["family"] and f["lds"] == i["lds"] + 64 * D and f["grid"] == i["grid"], (esz, D, f, i)
    # 513 columns, the non-RLE codecs
    assert planner.ask("encode", q=FLOAT, out_esz=4, **shape(1, 513, 513 * 16))["error"] == -4
    assert planner.ask("dense", q=FLOAT, out_esz=4, **shape(1, 513, 513 * 16))["error"] == -4
    assert planner.ask("encode", q=FLOAT, out_esz=4, **dict(shape(1, 16), codec=2))["error"] == -4


def test_planner_sweep_finds_no_other_family():
    """rowdata's NDIMS x four chunk lengths x four batch sizes x both widths, codecs, source sizes and no_fast: only enc_pair, enc_wide,
    enc_split and enc_generic, never dense_verbatim -- and the same queries without the float source give what they give today"""
    planner.available()
    queries, keys = [], []
    for esz in (1, 2):
        for D in NDIMS:
            for chunk_len in (13 * D, 16 * D, D * (16 * 4 + 3), rows16(D, esz)):
                for nchunks in (1, 64, 2048, 131072):
                    for codec in (0, 1):
                        for no_fast in (0, 1):
                            base = dict(shape(esz, D, chunk_len, nchunks), codec=codec, no_fast=no_fast)
                            for op in ("encode", "dense"):
                                queries += [(op, dict(base, q=FLOAT, out_esz=4)), (op, dict(base, q=FLOAT, out_esz=2)), (op, dict(base, q=0)), (op, base)]
                                keys += [(op, esz, D, chunk_len, nchunks, codec, no_fast)] * 4
    answers = planner.ask_many(queries)
    seen, verbatim_today = set(), 0
    for j in range(0, len(answers), 4):
        f4, f2, off, plain = answers[j:j + 4]
        op = keys[j][0]
        assert off == plain, (keys[j], off, plain)                                 # q = 0 is today's plan
        for f in (f4, f2):
            assert "error" not in f, (keys[j], f)
            enc = f["family"] if op == "encode" else f["enc"]
            assert enc in ("enc_pair", "enc_wide", "enc_split", "enc_generic") and enc not in EXCLUDED, (keys[j], f)
            if op == "dense":
                assert f["family"] in ("dense_fused", "dense_compact"), (keys[j], f)
            seen.add(enc)
        assert f4 == f2 or op == "encode", (keys[j], f4, f2)
        verbatim_today += op == "dense" and plain.get("family") == "dense_verbatim"
        if keys[j][6]:
            assert (f4["family"] if op == "encode" else f4["enc"]) == "enc_generic", (keys[j], f4)
    assert seen == {"enc_pair", "enc_wide", "enc_split", "enc_generic"}
    assert verbatim_today > 0                                                      # the sweep holds shapes the integer call hands to dense_verbatim
    line = planner.run("sweep\n")[-1]
    assert line.endswith("violations=0"), line


# ------------------------------------------------------------------ quant_params

def test_quant_params_is_numpy_float32_division():
    import torch
    from sprintz_amd import rowops
    dev = torch.device("cpu")
    assert rowops.quant_params(None, None, 4, dev) == (None, None)
    rng = np.random.default_rng(3)
    scale = (rng.uniform(1e-6, 1e6, 8) * rng.choice([-1, 1], 8)).astype(np.float64)
    offset = rng.normal(size=8) * 100
    inv, off = rowops.quant_params(scale, offset, 8, dev)
    assert inv.dtype == torch.float32 and off.dtype == torch.float32 and inv.is_contiguous() and tuple(inv.shape) == (8,)
    assert np.array_equal(inv.numpy().view(np.uint32), (np.float32(1) / scale.astype(np.float32)).view(np.uint32))
    assert np.array_equal(off.numpy(), offset.astype(np.float32))
    inv, off = rowops.quant_params(0.1, None, 3, dev)
    assert off is None and inv.tolist() == [float(np.float32(1) / np.float32(0.1))] * 3
    inv, off = rowops.quant_params(torch.tensor([2.0, 4.0], dtype=torch.float64), torch.tensor([1, 2]), 2, dev)
    assert inv.tolist() == [0.5, 0.25] and off.tolist() == [1.0, 2.0] and off.dtype == torch.float32
    inv, _ = rowops.quant_params(None, 1.5, 2, dev)
    assert inv is None
    for bad in (0.0, [1.0, 0.0], float("inf"), float("nan"), [1.0, float("-inf")], 1e39, 1e-60, 1e-39, torch.tensor([1.0, 0.0]), torch.tensor([float("nan"), 1.0])):
        with pytest.raises(ValueError):
            rowops.quant_params(bad, None, 2, dev)
    for bad in (float("inf"), [float("nan"), 0.0], torch.tensor([float("inf"), 0.0])):
        with pytest.raises(ValueError):
            rowops.quant_params(1.0, bad, 2, dev)
    for bad in ([1.0, 2.0, 3.0], torch.ones(5)):
        with pytest.raises(ValueError):
            rowops.quant_params(bad, None, 2, dev)
        with pytest.raises(ValueError):
            rowops.quant_params(None, bad, 2, dev)


def test_dequantize_params_round_trip_within_one_step():
    """compress_floats' model on datasets.dequantize_params' (scale, offset): "floor" lands within one step of datasets.quantize (which divides
    where this multiplies by a reciprocal), "nearest" within one step of the value itself"""
    import torch
    from sprintz_amd import datasets, rowops
    rng = np.random.default_rng(11)
    for dtype, W in ((np.uint8, 8), (np.uint16, 16)):
        m = rng.normal(size=(500, 6)) * rng.uniform(0.01, 1000.0, size=6) + rng.uniform(-500, 500, size=6)
        m[:, 0] = 3.25
        scale, offset = datasets.dequantize_params(m, dtype)
        inv, off = rowops.quant_params(scale, offset, 6, torch.device("cpu"))
        x = m.astype(np.float32).reshape(-1)
        qf = qm.compress_floats(x, x.size, 6, W, inv.numpy(), off.numpy(), floor=True).astype(np.int64).reshape(m.shape)
        assert np.abs(qf - datasets.quantize(m, dtype).astype(np.int64)).max() <= 1
        qn = qm.compress_floats(x, x.size, 6, W, inv.numpy(), off.numpy()).astype(np.float64).reshape(m.shape)
        back = qn * scale.astype(np.float64) + offset.astype(np.float64)
        slack = 8 * 2.0 ** -24 * (np.abs(m).max(axis=0) + np.maximum(1, m.max(axis=0) - m.min(axis=0)))
        assert np.all(np.abs(back - m) <= scale.astype(np.float64) + slack)
