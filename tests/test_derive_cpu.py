"""CPU tier of derive rows (sprintz_mi355x_derive_rows, ChunkedCodec.derive_rows / diff_rows): the symbols and their binding are there, every
validation return comes before the device is touched, the numpy model the GPU tier compares with (tests/derive_model.py) equals a
one-row-at-a-time brute force in Python integers and, for the float formats, torch's CPU expression bit for bit, rowops.derive_forms takes
every argument form and holds every form to linear_terms' bound, and the planner (sprintz_amd/csrc/plan.h, built with g++:
tests/plan_probe.cpp, asked with q=18 rows=K out_esz=...) sends the mode to decode_fast.h exactly on the one-column-a-lane mappings."""
import os

import numpy as np
import pytest

import derive_model as dm
import float_model as fm
import linear_model as lm
import planner
from derive_runner import check_refusals
from fixtures import buf_fixture, lib  # noqa: F401  (fixtures)
from rowdata import FLOAT_FAST_SHAPES as FAST_SHAPES, GENERIC_SHAPES, RAGGED_SHAPES

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = {1: np.uint8, 2: np.uint16}
Q_DERIVE = 18                                             # geom.h: kQueryDerive

buf = buf_fixture(16384)


def test_symbol_and_binding(lib):
    import ctypes as C
    for s in ("sprintz_mi355x_derive_rows", "sprintz_mi355x_derive_rows_tmp_bytes"):
        assert s in lib.EXPORTED_SYMBOLS and hasattr(lib.lib, s)
    assert len(lib.derive_rows.argtypes) == 20 and len(lib.derive_rows_tmp_bytes.argtypes) == 3
    assert lib.derive_rows_tmp_bytes.restype is C.c_uint64
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "sprintz_mi355x.h")).read()
    assert "int sprintz_mi355x_derive_rows(int codec, int elem_bytes, const void* d_comp, const uint64_t* d_offsets, uint64_t nchunks," in hdr
    assert "uint64_t sprintz_mi355x_derive_rows_tmp_bytes(int elem_bytes, uint64_t nchunks, uint16_t ndims);" in hdr
    assert (lib.DERIVE_I32, lib.DERIVE_F32, lib.DERIVE_F16, lib.DERIVE_BF16) == (0, 1 + lib.FLOAT_F32, 1 + lib.FLOAT_F16, 1 + lib.FLOAT_BF16)
    for name, v in (("SPRINTZ_DERIVE_I32", "0"), ("SPRINTZ_DERIVE_F32", "1"), ("SPRINTZ_DERIVE_F16", "2"), ("SPRINTZ_DERIVE_BF16", "3")):
        assert f"#define {name}" in hdr and hdr.split(f"#define {name}")[1].split()[0] == v
    assert lib.abi_version() == 7 and lib.KF_COUNT == 33          # additive: no new ABI version, no new kernel family
    geom = open(os.path.join(os.path.dirname(HERE), "sprintz_amd", "csrc", "geom.h")).read()
    assert f"kQueryDerive = {Q_DERIVE};" in geom
    # the scratch is the linear filter's, as it is
    for esz, n, D in ((1, 1, 1), (2, 5, 8), (1, 1000, 80), (2, 7, 512)):
        assert lib.derive_rows_tmp_bytes(esz, n, D) == lib.filter_linear_tmp_bytes(esz, n, D) == n * ((8 + 2 * D * esz + 7) & ~7)
    assert lib.derive_rows_tmp_bytes(3, 4, 8) == 0 and lib.derive_rows_tmp_bytes(2, 4, 513) == 0 and lib.derive_rows_tmp_bytes(2, 0, 8) == 0
    from sprintz_amd import ChunkedCodec
    assert callable(ChunkedCodec.derive_rows) and callable(ChunkedCodec.diff_rows)


def test_validation_comes_before_the_device(lib, buf):
    _, p = buf
    E = lib
    call = check_refusals(lib, p)
    import torch
    if not torch.cuda.is_available():
        assert call() == E.E_NO_DEVICE
        assert call(K=16) == E.E_NO_DEVICE and call(K=1, rets=None) == E.E_NO_DEVICE and call(flags=1) == E.E_NO_DEVICE
        assert call(u=p + 2048, tmp=p + 8192, bias=p + 3072, prev=p + 3074) == E.E_NO_DEVICE
        assert call(tmp=p + 8193) == E.E_NO_DEVICE                                # without a lag term the scratch is not looked at
        for fmt in (1, 2, 3):
            assert call(fmt=fmt, scale=p + 2048, offset=p + 3072) == E.E_NO_DEVICE
        assert call(fmt=2, out=p + 4098) == E.E_NO_DEVICE


# ------------------------------------------------------------------ the model

def extreme_forms(rng, esz, D, K, lag):
    """K forms: the first at B = 2^31 - 1 with random signs, then +-1 spreads, ones and random small weights"""
    top = (1 << (8 * esz)) - 1
    terms = D * (2 if lag else 1)
    wmax = ((1 << 31) - 1) // (top * terms)
    w = np.zeros((K, D), np.int64)
    u = np.zeros((K, D), np.int64) if lag else None
    bias = np.zeros(K, np.int64)
    w[0] = rng.choice([-wmax, wmax], D)
    if lag:
        u[0] = rng.choice([-wmax, wmax], D)
    bias[0] = (1 << 31) - 1 - lm.bound_B(esz, w[0], None if u is None else u[0])
    assert lm.bound_B(esz, w[0], None if u is None else u[0], bias[0]) == (1 << 31) - 1
    for k in range(1, K):
        w[k] = rng.integers(-3, 4, D)
        if lag:
            u[k] = -w[k] if k % 2 else rng.integers(-3, 4, D)
        bias[k] = int(rng.integers(-1000, 1000))
    return w, u, bias


@pytest.mark.parametrize("esz,D,chunk_len,n", RAGGED_SHAPES)
@pytest.mark.parametrize("lag", [False, True], ids=["nolag", "lag"])
def test_model_against_brute_force(esz, D, chunk_len, n, lag):
    """int64 matrix products wrapped to int32 against Python integers, a row and a form at a time: extremes of the element type (all-0 and all-max
    rows next to each other, so that a form at B = 2^31 - 1 reaches both ends), a lag term, a prev row, a partial last row (no row)"""
    rng = np.random.default_rng(n + lag)
    top = (1 << (8 * esz)) - 1
    x = rng.integers(0, top + 1, n).astype(DTYPES[esz])
    x[:D] = top
    x[D:2 * D] = 0
    x[2 * D:3 * D] = top
    for K in (1, 3, 16):
        w, u, bias = extreme_forms(rng, esz, D, K, lag)
        got = dm.sums(x, D, w, u, bias)
        assert got.shape == (n // D, K) and got.dtype == np.int64
        assert np.array_equal(got, dm.sums_brute(x, D, w, u, bias))
        assert got.min() >= -(1 << 31) and got.max() < (1 << 31)
        # B < 2^31: the wrapped sum is the plain integer
        v = x[:n // D * D].reshape(-1, D).astype(np.int64)
        plain = bias[None, :] + v @ w.T + (np.concatenate([v[:1], v[:-1]]) @ u.T if lag else 0)
        assert np.array_equal(got, plain)
        prev = rng.integers(0, top + 1, D).astype(DTYPES[esz])
        with_prev = dm.sums(x, D, w, u, bias, prev=prev)
        assert np.array_equal(with_prev, dm.sums_brute(x, D, w, u, bias, prev=prev))
        assert np.array_equal(with_prev[1:], got[1:])
        assert np.array_equal(with_prev[0], got[0]) == (not lag or np.array_equal(prev.astype(np.int64) @ u.T, v[0] @ u.T))
        # a form past the bound wraps as two's complement does
        big = w.copy()
        big[0] = (1 << 31) - 1
        assert np.array_equal(dm.sums(x, D, big, u, bias), dm.sums_brute(x, D, big, u, bias))
    # the diff of every column: numpy's, with row 0 prepended
    e = np.eye(D, dtype=np.int64)
    v = x[:n // D * D].reshape(-1, D).astype(np.int64)
    assert np.array_equal(dm.sums(x, D, e, -e), np.diff(v, axis=0, prepend=v[:1]))
    # self_rows: what the decode launch leaves for a chunk's first row
    R = chunk_len // D
    firsts = tuple(range(0, n // D, R))
    s = dm.sums(x, D, e, -e, self_rows=firsts)
    assert not s[list(firsts)].any() and np.array_equal(np.delete(s, firsts, 0), np.delete(np.diff(v, axis=0, prepend=v[:1]), firsts, 0))


SPECIAL_SUMS = [0, 1, -1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, -(1 << 24) - 1, -(1 << 24) - 3, (1 << 25) + 2, (1 << 25) + 6,
                (1 << 31) - 1, (1 << 31) - 64, (1 << 31) - 65, -(1 << 31), -(1 << 31) + 127, 65504, 65519, 65520, 2049, 2051, 257, 259, 0x10100, 0x10180, 0x10081]


@pytest.mark.parametrize("fmt", fm.FORMATS)
def test_model_floats_against_torch(fmt):
    """(s.to(float32) * scale + offset).to(dtype) on the CPU, bit for bit: |s| at and above 2^24 (the int32 -> float32 conversion rounds, ties to
    even), ties of the 16-bit formats, results that are inf and subnormal (float_model.PAIRS)"""
    import torch
    rng = np.random.default_rng(fmt)
    K = len(fm.PAIRS)
    s = np.concatenate([np.array(SPECIAL_SUMS, np.int64), rng.integers(-(1 << 31), 1 << 31, 4096), rng.integers(-70000, 70000, 4096)])
    s = np.repeat(s[:, None], K, axis=1)
    scale, offset = dm.form_params(K)
    got = dm.convert(s, fmt, scale, offset)
    dt = {fm.F32: torch.float32, fm.F16: torch.float16, fm.BF16: torch.bfloat16}[fmt]
    z = (torch.from_numpy(s.astype(np.int32)).to(torch.float32) * torch.from_numpy(scale) + torch.from_numpy(offset)).to(dt)
    want = z.view(torch.int32 if fmt == fm.F32 else torch.int16).numpy().view(fm.BITS_DTYPE[fmt])
    assert got.dtype == want.dtype and np.array_equal(got, want)
    f = (torch.from_numpy(s.astype(np.int32)).to(torch.float32) * torch.from_numpy(scale) + torch.from_numpy(offset)).numpy()
    assert np.isinf(f).any() and (np.abs(f[np.isfinite(f) & (f != 0)]).min() < 2.0 ** -126)      # inf and subnormal float32 results are among them
    # the conversion itself rounds to nearest even
    assert np.float32(np.int32((1 << 24) + 1)) == np.float32(1 << 24) and np.float32(np.int32((1 << 24) + 3)) == np.float32((1 << 24) + 4)
    # no parameters: scale 1, offset 0; the int32 format is the sum's own bits
    assert np.array_equal(dm.convert(s, fmt), dm.convert(s, fmt, np.ones(K), np.zeros(K)))
    assert np.array_equal(dm.convert(s, dm.I32).view(np.int32), s.astype(np.int32))


# ------------------------------------------------------------------ rowops

def test_derive_forms():
    import torch
    from sprintz_amd import rowops
    D = 5
    w, u, b = rowops.derive_forms([{0: 1, 1: -1}, 2, [1, 2, 3, 4, 5], torch.tensor([0, 0, 7, 0, 0])], None, 0, D, 2, "cpu")
    assert w.dtype == torch.int32 and w.shape == (4, D) and u is None and b.dtype == torch.int32 and b.tolist() == [0, 0, 0, 0]
    assert w.tolist() == [[1, -1, 0, 0, 0], [2] * 5, [1, 2, 3, 4, 5], [0, 0, 7, 0, 0]]
    w, u, b = rowops.derive_forms(torch.tensor([[1, 0, 0, 0, 0], [0, 0, 0, 0, -1]], dtype=torch.int64), [{0: -1}, 0], [5, -6], D, 1, "cpu")
    assert w.tolist() == [[1, 0, 0, 0, 0], [0, 0, 0, 0, -1]] and u.tolist() == [[-1, 0, 0, 0, 0], [0] * 5] and b.tolist() == [5, -6]
    assert u.dtype == torch.int32 and u.is_contiguous() and w.is_contiguous()
    w, u, b = rowops.derive_forms(np.eye(3, D, dtype=np.int64).tolist(), torch.tensor(-np.eye(3, D, dtype=np.int32)), 7, D, 2, "cpu")
    assert b.tolist() == [7, 7, 7] and (w + u).abs().sum() == 0
    # the bound, a form at a time: B = 2^31 - 1 is taken, 2^31 is not, and the refusal names the form
    for esz in (1, 2):
        top = (1 << (8 * esz)) - 1
        wmax = ((1 << 31) - 1) // (top * D)
        full = [wmax] * D
        bias = (1 << 31) - 1 - top * wmax * D
        assert lm.bound_B(esz, full, None, bias) == (1 << 31) - 1
        rowops.derive_forms([1, full], None, [0, bias], D, esz, "cpu")
        rowops.derive_forms([1, full], None, [0, -bias], D, esz, "cpu")
        with pytest.raises(ValueError, match="form 1 can reach 2147483648"):
            rowops.derive_forms([1, full], None, [0, bias + 1], D, esz, "cpu")
        with pytest.raises(ValueError, match="form 0 "):
            rowops.derive_forms([full, 1], [{0: 1}, 0], [bias, 0], D, esz, "cpu")
        # linear_terms keeps its own words and its own bound
        rowops.linear_terms(full, None, bias, None, None, D, esz, "cpu")
        with pytest.raises(ValueError, match="the linear form can reach 2147483648"):
            rowops.linear_terms(full, None, bias + 1, None, None, D, esz, "cpu")
    for bad in ([], [1] * 17, 1, {0: 1}, [[1, 2]], torch.ones(2, D), torch.ones(D, dtype=torch.int32), torch.ones((2, D + 1), dtype=torch.int32), [{D: 1}]):
        with pytest.raises((ValueError, TypeError)):
            rowops.derive_forms(bad, None, 0, D, 2, "cpu")
    assert rowops.derive_forms([1] * 16, None, 0, D, 2, "cpu")[0].shape == (16, D)
    with pytest.raises(ValueError):
        rowops.derive_forms([1, 2], [1], 0, D, 2, "cpu")                          # K lag forms, not one
    with pytest.raises(ValueError):
        rowops.derive_forms([1, 2], None, [1, 2, 3], D, 2, "cpu")                 # K biases


class FakeBatch:
    nchunks, total_len = 0, 0


def test_diff_rows_forms(monkeypatch):
    """diff_rows hands derive_rows e_c and -e_c for the columns it is given, all of them for None, and refuses more than 16"""
    import torch
    from sprintz_amd import ChunkedCodec
    seen = {}

    def fake(self, batch, forms, lag_forms=None, **kw):
        seen.update(forms=forms, lag=lag_forms, kw=kw)
        return "derived"
    monkeypatch.setattr(ChunkedCodec, "derive_rows", fake)
    cd = ChunkedCodec.__new__(ChunkedCodec)
    cd.ndims, cd.torch = 8, torch
    assert cd.diff_rows(FakeBatch()) == "derived"
    assert seen["forms"] == [{c: 1} for c in range(8)] and seen["lag"] == [{c: -1} for c in range(8)] and seen["kw"] == {}
    cd.diff_rows(FakeBatch(), [3, 0], dtype=torch.float32, scale=0.5, prev=[0] * 8)
    assert seen["forms"] == [{3: 1}, {0: 1}] and seen["lag"] == [{3: -1}, {0: -1}] and set(seen["kw"]) == {"dtype", "scale", "prev"}
    cd.diff_rows(FakeBatch(), torch.tensor([7]))
    assert seen["forms"] == [{7: 1}]
    for bad in ([], [8], [-1], [0.5], [True]):
        with pytest.raises(ValueError):
            cd.diff_rows(FakeBatch(), bad)
    with pytest.raises(ValueError):
        cd.diff_rows(FakeBatch(), [0], forms=[1])
    cd.ndims = 17
    with pytest.raises(ValueError, match="at most 16 columns"):
        cd.diff_rows(FakeBatch())
    with pytest.raises(ValueError, match="at most 16 columns"):
        cd.diff_rows(FakeBatch(), list(range(17)))
    cd.diff_rows(FakeBatch(), list(range(16)))
    assert len(seen["forms"]) == 16


# ------------------------------------------------------------------ the planner

@pytest.fixture(scope="module")
def plan():
    planner.available()
    return lambda **fields: planner.ask("decode", q=Q_DERIVE, **fields)


def named_chunk_len(D):
    return D * (16 * 4 + 3)


PLANNER_SHAPES = [(esz, D, 67) for esz, D in FAST_SHAPES + GENERIC_SHAPES] + [(2, 4, 80), (1, 6, 80), (1, 8, 80), (1, 64, 67), (2, 33, 80), (2, 40, 67), (1, 65, 80),
                                                                             (2, 65, 80), (2, 300, 80)]


@pytest.mark.parametrize("esz,D,R", PLANNER_SHAPES)
def test_planner_family(plan, esz, D, R):
    """decode_fast.h on uint16 x 8 / 16 / 24 / 64 and uint8 x 16 / 64 (and the other one-column-a-lane mappings) for every K and every output
    element; the generic kernel for 65 / 80 / 128 / 256 / 300 columns -- two and four columns a lane are not built for this mode -- for the
    low-dim shapes, under NO_FAST and for an output off the 16-byte grid"""
    chunk_len = D * R
    seen = set()
    for general in (0, 1):
        for K in (1, 2, 3, 8, 16):
            for osz in (2, 4):
                for no_fast in (0, 1):
                    for cpg in (1, 3):
                        for out_lo in (0, osz, 8):
                            got = plan(esz=esz, D=D, chunk_len=chunk_len, nchunks=5, codec=1, rows=K, out_esz=osz, general=general, no_fast=no_fast,
                                       chunks_per_group=cpg, out_lo=out_lo)
                            want = dm.fast_takes(esz, D, chunk_len, K, osz, general, no_fast, out_lo)
                            assert got.get("family") == ("dec_fast" if want else "dec_generic"), (got, K, osz, general, no_fast, out_lo)
                            if want:
                                plain = planner.ask("decode", esz=esz, D=D, chunk_len=chunk_len, nchunks=4096, codec=1, general=general, chunks_per_group=cpg)
                                assert plain["family"] == "dec_fast"             # a shape the plain decode runs there
                                stride = dm.fast_stride(esz, D, K, osz)
                                assert got["cpl"] == 1 and got["dp"] == plain["dp"] and got["lds_group_stride"] == stride >= plain["lds_group_stride"], (got, plain)
                                assert stride - plain["lds_group_stride"] == max(0, 8 * K * osz - ((8 * D * esz + 15) & ~15))
                                groups = 256 // got["dp"]
                                assert got["table_off"] == stride * groups and got["lds"] == stride * groups + K * D * 8 <= 80 * 1024, got
                                assert got["chunks_per_group"] == cpg and got["grid"] == -(--(-5 // cpg) * got["dp"] // 256), got
                            else:
                                assert got["lds"] == 0 and got["vec_store"] == 0 and got["grid"] == -(-5 * (1 << got["log2DP"]) // 256), got
                            if not no_fast and not out_lo:
                                seen.add(got["family"])
    if (esz, D) in ((2, 4), (2, 8), (2, 16), (2, 24), (2, 33), (2, 40), (2, 64), (1, 8), (1, 16), (1, 64)) or (esz, D, R) == (1, 6, 80):
        assert seen == {"dec_fast"}
    else:
        assert seen == {"dec_generic"}


def test_planner_refusals(plan):
    for esz, D in ((2, 8), (1, 16), (2, 1), (1, 80)):
        for K in (0, 17, 1000):
            got = plan(esz=esz, D=D, chunk_len=named_chunk_len(D), nchunks=5, codec=0, rows=K, out_esz=4)
            assert got.get("error") == -1 and "derive_rows" in got["what"], got      # SPRINTZ_E_INVALID
    for codec in (2, 3):
        got = plan(esz=1, D=8, chunk_len=8 * 67, nchunks=5, codec=codec, rows=2, out_esz=4)
        assert got.get("error") == -4 and "derive_rows" in got["what"], got
    assert plan(esz=1, D=513, chunk_len=513 * 16, nchunks=5, codec=0, rows=2, out_esz=4).get("error") == -4


def test_planner_reach_counts_derived_bytes(plan):
    """the wave's chunks lie within 32-bit offsets of its first: 4096 derived slots below 0xf0000000 bytes -- both sides of the edge at uint16 x 8,
    where two int32 values a row stay inside and three do not, and four 16-bit floats do where five do not"""
    D, R = 8, 100000
    assert R * 2 * 4 * 4096 < 0xf0000000 <= R * 3 * 4 * 4096
    for K, fam in ((1, "dec_fast"), (2, "dec_fast"), (3, "dec_generic"), (8, "dec_generic"), (16, "dec_generic")):
        assert plan(esz=2, D=D, chunk_len=D * R, nchunks=5, codec=1, rows=K, out_esz=4)["family"] == fam
    assert R * 4 * 2 * 4096 < 0xf0000000 <= R * 5 * 2 * 4096
    assert plan(esz=2, D=D, chunk_len=D * R, nchunks=5, codec=1, rows=4, out_esz=2)["family"] == "dec_fast"
    assert plan(esz=2, D=D, chunk_len=D * R, nchunks=5, codec=1, rows=5, out_esz=2)["family"] == "dec_generic"


def test_planner_leaves_the_other_modes_alone():
    """rows and out_esz mean nothing to the plain decode, and the linear filter's plan is the one it had"""
    planner.available()
    base = dict(esz=2, D=8, chunk_len=5120, nchunks=4096, codec=1)
    assert planner.ask("decode", **base) == planner.ask("decode", rows=2, out_esz=4, **base)
    assert planner.ask("decode", q=12, **base)["family"] == "dec_fast" and planner.ask("decode", q=12, **base)["table_off"] == 0
