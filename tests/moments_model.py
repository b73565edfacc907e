"""numpy / Python-int model of moments rows (sprintz_mi355x_moments_rows, include/sprintz_mi355x.h), applied to the ORIGINAL input --
decode is lossless and pinned elsewhere -- a one-row-at-a-time brute force of the same definition in Python ints, and the exact
rationals (fractions.Fraction) of what ChunkedCodec.moments_rows derives from the integer sums.

chunk_len % D == 0; R = chunk_len // D rows a chunk slot, MB = ceil(R / 8) mask bytes a chunk slot, W rows a window, nwin = ceil(R / W)
windows a chunk slot.  Which rows exist and are selected is aggregate_model.selected's business (mask None: every existing row).  Window
w of chunk c takes the selected rows r with r // W == w: their number, and per column d the sum of x_d, of x_d^2 and of x_d * x_ref.
Every value is an exact unsigned integer below 2^62; a window with no selected row holds zeros."""
import math
from fractions import Fraction

import numpy as np

import aggregate_model as am
import filter_model as fm

U = 2.0 ** -53                  # float64's unit roundoff


def all_rows(n, chunk_len, D):
    """the mask of mask=None: every bit set (aggregate_model.selected drops the rows that do not exist)"""
    R, MB = fm.geometry(chunk_len, D)
    return np.full((len(fm.chunk_counts(n, chunk_len)), MB), 0xFF, np.uint8)


def moments_rows(x, chunk_len, D, mask, W, ref=0):
    """x: the flat original array; mask: uint8 [nchunks, MB] or None.  -> dict: sum / sumsq / cross (uint64) [nchunks, nwin, D], count
    (uint32) [nchunks, nwin]"""
    assert chunk_len % D == 0 and W % 8 == 0 and W >= 8 and 0 <= ref < D
    x = np.asarray(x).ravel()
    R = chunk_len // D
    nwin = -(-R // W)
    sel = am.selected(all_rows(x.size, chunk_len, D) if mask is None else mask, x.size, chunk_len, D)
    nchunks = sel.shape[0]
    # every chunk slot padded to nwin * W rows; a row that is not selected holds 0, the identity of every sum
    v = np.zeros((nchunks, nwin * W, D), np.uint64)
    for c, ne in enumerate(fm.chunk_counts(x.size, chunk_len)):
        v[c, :ne // D] = x[c * chunk_len:c * chunk_len + ne // D * D].reshape(-1, D)
    v[:, :R][~sel] = 0
    v = v.reshape(nchunks, nwin, W, D)
    s = np.zeros((nchunks, nwin * W), bool)
    s[:, :R] = sel
    return {"sum": v.sum(axis=2), "sumsq": (v * v).sum(axis=2), "cross": (v * v[..., ref:ref + 1]).sum(axis=2),
            "count": s.reshape(nchunks, nwin, W).sum(axis=2).astype(np.uint32)}


def moments_rows_brute(x, chunk_len, D, mask, W, ref=0):
    """the same definition, one row at a time, in Python ints -> dict of nested lists [nchunks][nwin][D] / [nchunks][nwin]"""
    x = np.asarray(x).ravel()
    R = chunk_len // D
    nwin = -(-R // W)
    lens = fm.chunk_counts(x.size, chunk_len)
    sm = [[[0] * D for _ in range(nwin)] for _ in lens]
    sq = [[[0] * D for _ in range(nwin)] for _ in lens]
    cr = [[[0] * D for _ in range(nwin)] for _ in lens]
    cnt = [[0] * nwin for _ in lens]
    for c, ne in enumerate(lens):
        for r in range(R):
            if (r + 1) * D > ne or (mask is not None and not (int(mask[c][r >> 3]) >> (r & 7)) & 1):
                continue
            w = r // W
            cnt[c][w] += 1
            xr = int(x[c * chunk_len + r * D + ref])
            for d in range(D):
                v = int(x[c * chunk_len + r * D + d])
                sm[c][w][d] += v
                sq[c][w][d] += v * v
                cr[c][w][d] += v * xr
    return {"sum": sm, "sumsq": sq, "cross": cr, "count": cnt}


def global_windows(x, chunk_len, D, mask, W, ref=0):
    """windows over the batch's rows (chunk c holds batch rows [c R, (c + 1) R)): window w covers rows [w W, (w + 1) W), w <
    ceil(ceil(n / D) / W).  -> dict of sum / sumsq / cross [nwindows, D] and count [nwindows], all int64"""
    x = np.asarray(x).ravel()
    R = chunk_len // D
    sel = am.selected(all_rows(x.size, chunk_len, D) if mask is None else mask, x.size, chunk_len, D)
    rows = -(-x.size // D)
    nw = -(-rows // W)
    out = {k: np.zeros((nw, D), np.int64) for k in ("sum", "sumsq", "cross")}
    out["count"] = np.zeros(nw, np.int64)
    for c in range(sel.shape[0]):
        r = np.flatnonzero(sel[c])
        if r.size == 0:
            continue
        v = x[c * chunk_len:(c + 1) * chunk_len]
        v = v[:v.size // D * D].reshape(-1, D)[r].astype(np.int64)
        w = (c * R + r) // W
        np.add.at(out["sum"], w, v)
        np.add.at(out["sumsq"], w, v * v)
        np.add.at(out["cross"], w, v * v[:, ref:ref + 1])
        np.add.at(out["count"], w, 1)
    return out


def exact_derived(n, S, Q, P=None, Sr=None, Qr=None, ddof=0):
    """one entry's exact values from its integer sums (Python ints): n rows, S = sum x, Q = sum x^2 and, with the reference column,
    P = sum x y, Sr = sum y, Qr = sum y^2.  -> dict of Fractions (corr2: the SQUARE of the correlation, with sign: its sign), or
    None where the value does not exist (n == 0, n <= ddof, a variance of 0)"""
    n, S, Q = int(n), int(S), int(Q)
    out = {"mean": Fraction(S, n) if n else None, "var": None, "cov": None, "corr2": None, "sign": 0}
    if n > ddof:
        out["var"] = Fraction(n * Q - S * S, n * (n - ddof))
    if P is not None:
        P, Sr, Qr = int(P), int(Sr), int(Qr)
        if n > ddof:
            out["cov"] = Fraction(n * P - S * Sr, n * (n - ddof))
        vx, vy, cxy = n * Q - S * S, n * Qr - Sr * Sr, n * P - S * Sr
        if n and vx and vy:
            out["corr2"] = Fraction(cxy * cxy, vx * vy)
            out["sign"] = (cxy > 0) - (cxy < 0)
    return out


def corr_float(e):
    """exact_derived's correlation rounded to float64: sign * sqrt(corr2), the root taken on integers scaled by 2^200 (so its own
    error is far below 2^-53)"""
    if e["corr2"] is None:
        return float("nan")
    f = e["corr2"]
    root = Fraction(math.isqrt((f.numerator << 400) // f.denominator), 1 << 200)
    return e["sign"] * float(root)


def corr_bound(vx, vy):
    """the bound on |corr - exact| for exact variances vx, vy that test_moments_derived_values derives in its docstring"""
    v = min(vx, vy)
    return 32 * U if v >= 1 else (12 * (1 + 1 / float(v)) + 3) * U
