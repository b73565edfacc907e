"""CPU tests of sprintz_amd/rowops.py, the host-side rules ChunkedCodec's row operations share: the kernel window plan and the fold of
its per-chunk results into windows over the batch's rows against the numpy models, the moments' derived values against exact rationals,
bounds and offsets as tensors, the default bin shift and the first damaged chunk.  CPU torch tensors only: no library, no device.  The
module is loaded from its file -- importing the package would load the library."""
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import aggregate_model as am
import filter_model as fm
import groupby_model as gm
import histogram_model as hm
import moments_model as mm
import window_model as wm
from moments_model import U, corr_bound

_spec = importlib.util.spec_from_file_location(
    "sprintz_amd_rowops", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sprintz_amd", "rowops.py"))
rowops = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rowops)

CPU = torch.device("cpu")
TORCH = {1: torch.uint8, 2: torch.uint16}
NP = {1: np.uint8, 2: np.uint16}


class Refusal(Exception):
    """stands in for SprintzError: (code, message)"""
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def test_plan_windows_every_small_shape():
    """R in 1..40, window_rows in 1..96 and None, both modes: window_model.kernel_window's plan wherever it has one -- except W == R,
    where one window a chunk (ceil(R / 8) * 8 rows, nothing folds) serves every R -- a ValueError everywhere else, and nwin ==
    ceil(R / kw) throughout"""
    D = 3
    served = refused = 0
    for R in range(1, 41):
        r8 = -(-R // 8) * 8
        assert rowops.plan_windows(R, None, True) == (r8, 1, 1)
        assert rowops.plan_windows(R, None, False) == (r8, 1, 1)
        for W in range(1, 97):
            assert rowops.plan_windows(R, W, True) == (W, 1, -(-R // W)), (R, W)
            want = (r8, 1) if W == R else wm.kernel_window(R * D, D, W)
            if want is None:
                assert W % R and R % W
                with pytest.raises(ValueError, match=f"chunk rows {R} .* window_rows {W}"):
                    rowops.plan_windows(R, W, False)
                refused += 1
            else:
                kw, fold, nwin = rowops.plan_windows(R, W, False)
                assert (kw, fold) == want and nwin == -(-R // kw), (R, W)
                assert kw * nwin >= R and (fold == 1 or nwin == 1), (R, W)
                served += 1
    assert served > 200 and refused > 2000
    for per_chunk in (False, True):
        for W in (0, -8):                                   # (-8 would reach the library as a multiple of 8)
            with pytest.raises(ValueError, match="positive"):
                rowops.plan_windows(16, W, per_chunk)


def _t(a, esz=None):
    """numpy -> torch: sums and counts as int64, samples in their own dtype"""
    return torch.from_numpy(np.ascontiguousarray(a if esz else a.astype(np.int64)))


FOLD_SHAPES = [(3, 8, 24, 61), (5, 12, 36, 100), (2, 16, 16, 33), (4, 24, 8, 50)]     # (D, R, W, rows): fold 3 and a padded last window, fold
#                                                                                      3 at R % 8 != 0, W == R, and three windows a chunk


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("D,R,W,rows", FOLD_SHAPES)
def test_fold_windows_against_models(esz, D, R, W, rows):
    """per-chunk windows of the numpy models at the planned kernel window, folded: the models' windows over the batch's rows, bit for
    bit -- the last chunk is short and the last row partial"""
    rng = np.random.default_rng(1000 * esz + rows)
    total, chunk_len = rows * D - 1, R * D
    x = rng.integers(0, 1 << (8 * esz), size=total).astype(NP[esz])
    x[rng.integers(0, total, size=4)] = (1 << (8 * esz)) - 1
    n = -(-total // chunk_len)
    assert total % chunk_len and total % D
    kw, fold, nwin = rowops.plan_windows(R, W, False)
    args = (n, nwin, D, W, fold, total, esz, TORCH[esz])

    mn, mx, sm = wm.chunk_windows(x, chunk_len, D, kw)
    got = rowops.fold_windows({"min": _t(mn, esz), "max": _t(mx, esz), "sum": _t(sm)}, *args)
    want = wm.global_windows(x, D, W)
    assert list(got) == ["min", "max", "sum"]
    assert got["min"].dtype == got["max"].dtype == TORCH[esz] and got["sum"].dtype == torch.int64
    for k in got:
        assert np.array_equal(got[k].numpy(), want[k]), k

    mask = rng.integers(0, 256, size=(n, -(-R // 8))).astype(np.uint8)
    mask[n // 2] = 0                                        # a chunk without a selected row: the identities fold
    pc = am.aggregate_rows(x, chunk_len, D, mask, kw)
    got = rowops.fold_windows({"min": _t(pc["min"], esz), "max": _t(pc["max"], esz), "sum": _t(pc["sum"]), "count": _t(pc["count"])}, *args)
    want = am.global_windows(x, chunk_len, D, mask, W)
    for k in ("min", "max", "sum", "count"):
        assert got[k].numpy().dtype == want[k].dtype and np.array_equal(got[k].numpy(), want[k]), k

    for ref in (0, D - 1):
        pc = mm.moments_rows(x, chunk_len, D, mask, kw, ref)
        got = rowops.fold_windows({k: _t(pc[k]) for k in ("sum", "sumsq", "cross", "count")}, *args)
        want = mm.global_windows(x, chunk_len, D, mask, W, ref)
        for k in ("sum", "sumsq", "cross", "count"):
            assert got[k].dtype == torch.int64 and np.array_equal(got[k].numpy(), want[k]), (k, ref)


def test_fold_windows_empty_batch():
    for fold, W in ((1, 8), (3, 24)):
        got = rowops.fold_windows({"min": torch.empty((0, 1, 2), dtype=torch.uint16), "count": torch.empty((0, 1), dtype=torch.int64)},
                                  0, 1, 2, W, fold, 0, 2, torch.uint16)
        assert tuple(got["min"].shape) == (0, 2) and got["min"].dtype == torch.uint16 and tuple(got["count"].shape) == (0,)


DERIVED = ("mean", "var", "std", "cov", "corr")


def test_derive_moments_against_exact_rationals():
    """test_moments_derived_values' bounds (u = 2^-53: u |exact| for the mean, 6 u (|exact| + 1) for var and cov, 8 u (exact + 1) on std^2,
    corr_bound for corr) on windows of 0, 1, 2 and 1 720 rows, ddof 0 and 1; column 1 is constant, column 2 is column 0 again, column 3
    its mirror image and columns 4 .. 7 hold 65534 or 65535 alone -- where n Q - S^2 in float64 fails the bound the pivot keeps"""
    rng = np.random.default_rng(77)
    D, sizes = 8, (0, 1, 2, 1720)
    rows = []
    for n in sizes:
        x = np.mod(np.cumsum(rng.integers(-300, 301, size=(n, D)), axis=0) + rng.integers(0, 65536, size=(1, D)), 65536)
        x[:, 1] = 4660
        x[:, 2] = x[:, 0]
        x[:, 3] = 65535 - x[:, 0]
        x[:, 4:] = 65534 + rng.integers(0, 2, size=(n, 4))
        rows.append(x.astype(np.int64))
    tested = {"corr": 0, "corr below 1": 0, "nan corr": 0}
    naive_fails = 0
    for ref in (0, 1, 5):
        ints = {"count": torch.tensor([len(x) for x in rows], dtype=torch.int64),
                "sum": torch.from_numpy(np.stack([x.sum(axis=0) for x in rows])),
                "sumsq": torch.from_numpy(np.stack([(x * x).sum(axis=0) for x in rows])),
                "cross": torch.from_numpy(np.stack([(x * x[:, ref:ref + 1]).sum(axis=0) for x in rows]))}
        for ddof in (0, 1):
            got = rowops.derive_moments(dict(ints), DERIVED, ref, ddof)
            assert list(got) == list(DERIVED)
            assert all(v.dtype == torch.float64 and tuple(v.shape) == (len(sizes), D) for v in got.values())
            got = {k: v.numpy() for k, v in got.items()}
            for w, n in enumerate(sizes):
                Sr, Qr = int(ints["sum"][w, ref]), int(ints["sumsq"][w, ref])
                for d in range(D):
                    S, Q, P = int(ints["sum"][w, d]), int(ints["sumsq"][w, d]), int(ints["cross"][w, d])
                    e = mm.exact_derived(n, S, Q, P, Sr, Qr, ddof)
                    msg = (ref, ddof, n, d)
                    if e["mean"] is None:
                        assert n == 0 and np.isnan(got["mean"][w, d]), msg
                    else:
                        assert abs(Fraction(got["mean"][w, d]) - e["mean"]) <= Fraction(U) * abs(e["mean"]), msg
                    for k in ("var", "cov"):
                        if e[k] is None:
                            assert n <= ddof and np.isnan(got[k][w, d]), (k,) + msg
                        else:
                            assert abs(Fraction(got[k][w, d]) - e[k]) <= 6 * Fraction(U) * (abs(e[k]) + 1), (k, got[k][w, d], float(e[k])) + msg
                    if e["var"] is None:
                        assert np.isnan(got["std"][w, d]), msg
                    else:
                        assert abs(Fraction(got["std"][w, d]) ** 2 - e["var"]) <= 8 * Fraction(U) * (e["var"] + 1), msg
                    if e["corr2"] is None:
                        assert np.isnan(got["corr"][w, d]), msg
                        tested["nan corr"] += n > 0
                    else:
                        vx, vy = Fraction(n * Q - S * S, n * n), Fraction(n * Qr - Sr * Sr, n * n)
                        bound = corr_bound(vx, vy)
                        assert abs(got["corr"][w, d] - mm.corr_float(e)) <= bound, (got["corr"][w, d], mm.corr_float(e)) + msg
                        assert abs(got["corr"][w, d]) <= 1.0 + bound, msg
                        tested["corr" if vx >= 1 and vy >= 1 else "corr below 1"] += 1
                    if n == 1720 and d >= 4 and ddof == 0 and ref == 0:
                        naive = (float(n) * float(Q) - float(S) * float(S)) / (float(n) * float(n))
                        naive_fails += abs(Fraction(naive) - e["var"]) > 6 * Fraction(U) * (e["var"] + 1)
    assert all(v > 0 for v in tested.values()), tested
    assert naive_fails > 0
    # the columns the derivation speaks of: identical, mirrored and constant
    got = rowops.derive_moments(dict(ints, cross=torch.from_numpy(np.stack([(x * x[:, 0:1]).sum(axis=0) for x in rows]))), ("corr",), 0, 0)
    corr = got["corr"].numpy()[3]
    assert abs(corr[2] - 1) <= 32 * U and abs(corr[3] + 1) <= 32 * U and np.isnan(corr[1])
    # only what the ops need has to be there
    assert list(rowops.derive_moments({"count": ints["count"], "sum": ints["sum"]}, ("mean",), None, 0)) == ["mean"]


@pytest.mark.parametrize("esz", [1, 2])
def test_elem_tensor(esz):
    D, dt, top = 3, TORCH[esz], (1 << (8 * esz)) - 1

    def et(v, name="v", open_end=None):
        t = rowops.elem_tensor(v, D, esz, dt, CPU, name, open_end)
        assert t.dtype == dt and tuple(t.shape) == (D,) and t.is_contiguous() and t.device == CPU
        return t.numpy().astype(np.int64).tolist()

    assert et(7) == [7, 7, 7] and et(np.int64(top)) == [top] * 3 and et([0, 1, top]) == [0, 1, top]
    assert et([5, None, 9], open_end=0) == [5, 0, 9] and et((None, None, 1), open_end=top) == [top, top, 1]
    assert et(None, open_end=top) == [top] * 3
    with pytest.raises(TypeError):
        et([5, None, 9])                                    # an offset has no open end
    same = torch.from_numpy(np.array([top, 0, top - 1], NP[esz]))
    assert et(same) == [top, 0, top - 1] and et(same, open_end=0) == [top, 0, top - 1]
    assert et(same.reshape(3, 1).expand(3, 2)[:, 0]) == [top, 0, top - 1]      # not contiguous going in
    wide = torch.tensor([-1, (top + 1) * 3 + 5, top], dtype=torch.int64)
    assert et(wide) == [top, 5, top]                        # modulo 2^W
    assert et(torch.tensor([200, 100, 7], dtype=torch.int32)) == [200, 100, 7]
    with pytest.raises(ValueError, match=f"lo must hold 3 entries of {dt}"):
        et(wide, "lo", open_end=0)                          # a bound is not wrapped
    with pytest.raises(ValueError, match="v must hold 3 entries"):
        et(torch.zeros(4, dtype=dt))
    with pytest.raises(ValueError, match="hi must be a scalar or have 3 entries, not 2"):
        et([1, 2], "hi")
    for bad in (top + 1, -1, [0, top + 1, 0]):
        with pytest.raises(ValueError, match=f"entries must be in 0..{top}"):
            et(bad)


@pytest.mark.parametrize("esz", [1, 2])
def test_filter_bounds_open_ends(esz):
    """a column with neither bound: the whole range under "all", an empty interval under "any" -- as filter_model.neutral has it"""
    D, dt, top = 4, TORCH[esz], (1 << (8 * esz)) - 1
    lo, hi = [3, None, None, 9], [None, 200, None, None]
    for mode, code in (("all", fm.ALL), ("any", fm.ANY)):
        lo_t, hi_t = rowops.filter_bounds(lo, hi, mode, D, esz, dt, CPU)
        nlo, nhi = fm.neutral(esz, code)
        assert lo_t.numpy().tolist() == [3, 0, nlo, 9] and hi_t.numpy().tolist() == [top, 200, nhi, top], mode
        assert lo_t.dtype == hi_t.dtype == dt
    assert lo == [3, None, None, 9] and hi == [None, 200, None, None]          # the caller's lists stay
    lo_t, hi_t = rowops.filter_bounds(None, None, "any", D, esz, dt, CPU)       # scalars: every column
    assert lo_t.numpy().tolist() == [top] * D and hi_t.numpy().tolist() == [0] * D
    lo_t, hi_t = rowops.filter_bounds(1, 0, "any", D, esz, dt, CPU)
    assert lo_t.numpy().tolist() == [1] * D and hi_t.numpy().tolist() == [0] * D
    given = torch.from_numpy(np.array([1, 2, 3, 4], NP[esz]))
    lo_t, hi_t = rowops.filter_bounds(given, None, "any", D, esz, dt, CPU)      # a tensor names every bound: nothing to rewrite
    assert lo_t.numpy().tolist() == [1, 2, 3, 4] and hi_t.numpy().tolist() == [top] * D
    with pytest.raises(ValueError, match="hi must be a scalar or have 4 entries, not 3"):
        rowops.filter_bounds(0, [1, 2, 3], "any", D, esz, dt, CPU)
    with pytest.raises(ValueError, match=f"lo entries must be in 0..{top}"):
        rowops.filter_bounds(top + 1, None, "all", D, esz, dt, CPU)


def test_default_shift_equals_the_models():
    nbins = sorted({b for p in range(17) for b in ((1 << p) - 1, 1 << p, (1 << p) + 1) if 1 <= b <= 65536})
    assert nbins[0] == 1 and nbins[-1] == 65536 and len(nbins) > 40
    for esz in (1, 2):
        for b in nbins:
            assert rowops.default_shift(8 * esz, b) == hm.default_shift(esz, b) == gm.default_shift(esz, b), (esz, b)


def test_first_bad_and_raise_damaged():
    rets = torch.tensor([5120, 5120, -3, 100, -7, -1], dtype=torch.int64)
    assert rowops.first_bad(rets, 6) == 2                   # the first of several
    assert rowops.first_bad(rets, 2) is None                # what lies behind n does not count
    assert rowops.first_bad(rets[:2], 2) is None and rowops.first_bad(rets, 0) is None
    assert rowops.first_bad(torch.empty(0, dtype=torch.int64), 0) is None
    assert rowops.first_bad(rets[4:], 2) == 0
    with pytest.raises(Refusal, match=r"^select_rows: chunk 2 is damaged \(decoder returned -3\)$") as e:
        rowops.raise_damaged("select_rows", rets, 6, Refusal)
    assert e.value.code == -3
    rowops.raise_damaged("select_rows", rets, 2, Refusal)   # nothing damaged: returns
    rowops.raise_damaged("select_rows", rets, 0, Refusal)


def test_chunk_rows_mask_and_ops():
    assert rowops.chunk_rows(5120, 8, "select_rows") == (640, 80) == fm.geometry(5120, 8)
    assert rowops.chunk_rows(1024, 80) == (13, 2) == fm.geometry(1024, 80)     # nobody asked for whole rows
    with pytest.raises(ValueError, match=r"^groupby_rows needs chunk_len % ndims == 0 \(1024 % 80\): rows must not straddle chunks$"):
        rowops.chunk_rows(1024, 80, "groupby_rows")
    with pytest.raises(ValueError, match=r"^ids need chunk_len % ndims == 0 "):
        rowops.chunk_rows(1024, 80, "ids", verb="need")
    mask = torch.zeros((4, 6), dtype=torch.uint8)
    assert rowops.check_mask(mask, 4, 6, CPU) is mask and rowops.check_mask(mask[:, ::2], 4, 3, CPU).is_contiguous()
    for bad in (mask, mask[:, :3].to(torch.int8), mask[:, :3].numpy(), None):
        with pytest.raises(ValueError, match="mask must be a uint8 tensor of 4 x 3 bytes on cpu"):
            rowops.check_mask(bad, 4, 3, CPU)
    allowed = ("count", "sum")
    assert rowops.normalise_ops("sum", allowed, "count / sum") == ("sum",)
    assert rowops.normalise_ops(["sum", "count"], allowed, "count / sum") == ("sum", "count")
    for bad in ((), ("sum", "median")):
        with pytest.raises(ValueError, match="ops must be a non-empty subset of count / sum, not"):
            rowops.normalise_ops(bad, allowed, "count / sum")
