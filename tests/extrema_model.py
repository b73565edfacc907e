"""numpy model of extrema rows (sprintz_mi355x_extrema_rows, include/sprintz_mi355x.h), applied to the ORIGINAL input -- decode is
lossless and pinned elsewhere -- a one-row-at-a-time brute force of the same definition, and the windows over the batch's rows that
ChunkedCodec.extrema_rows folds them into.

chunk_len % D == 0; R = chunk_len // D rows a chunk slot, MB = ceil(R / 8) mask bytes a chunk slot, W rows a window, nwin = ceil(R / W)
windows a chunk slot.  Row r of chunk c EXISTS if all D of its elements lie inside the chunk's element count (a partial last row is not
a row); it is SELECTED if it exists and (mask is None or bit r & 7 of mask[c, r >> 3] is set).  Window w of chunk c takes the selected
rows r with r // W == w: per column their unsigned min / max and the chunk-relative row of the FIRST of them that holds it (numpy's tie
rule), the column's value in the first and in the last of them, those two rows, and their number.  A window with no selected row holds
min all ones, max 0, every row NO_ROW, first = last = 0, count 0."""
import numpy as np

import aggregate_model as am
import filter_model as fm

NO_ROW = 0xFFFFFFFF


def selected(mask, n, chunk_len, D):
    """-> bool [nchunks, R]: the rows that exist and whose bits are set (mask None: every bit is)"""
    R = chunk_len // D
    if mask is None:
        mask = np.full((len(fm.chunk_counts(n, chunk_len)), -(-R // 8)), 0xFF, np.uint8)
    return am.selected(mask, n, chunk_len, D)


def extrema_rows(x, chunk_len, D, mask, W):
    """x: the flat original array; mask: uint8 [nchunks, MB] or None.  -> dict: min / max / first / last (x's dtype) and argmin / argmax
    (uint32) [nchunks, nwin, D], rows (uint32) [nchunks, nwin, 2], count (uint32) [nchunks, nwin]"""
    assert chunk_len % D == 0 and W % 8 == 0 and W >= 8
    x = np.asarray(x).ravel()
    R = chunk_len // D
    nwin = -(-R // W)
    sel = selected(mask, x.size, chunk_len, D)
    nchunks = sel.shape[0]
    top = am.ident_min(x.dtype.itemsize)
    v = np.zeros((nchunks, nwin * W, D), np.int64)
    s = np.zeros((nchunks, nwin * W), bool)
    s[:, :R] = sel
    for c, ne in enumerate(fm.chunk_counts(x.size, chunk_len)):
        v[c, :ne // D] = x[c * chunk_len:c * chunk_len + ne // D * D].reshape(-1, D)
    v = v.reshape(nchunks, nwin, W, D)
    s = s.reshape(nchunks, nwin, W)
    s4 = s[..., None]
    any_ = s.any(axis=2)                                    # [nchunks, nwin]
    row0 = (np.arange(nwin, dtype=np.int64) * W)[None, :, None]
    # a row that is not selected holds a value no selected row can beat: top + 1 under the minimum, -1 under the maximum -- so argmin /
    # argmax (first occurrence) land on a selected row wherever there is one
    lo = np.where(s4, v, top + 1)
    hi = np.where(s4, v, -1)
    amin = lo.argmin(axis=2) + row0
    amax = hi.argmax(axis=2) + row0
    first = s.argmax(axis=2)                                # window-relative
    last = W - 1 - s[:, :, ::-1].argmax(axis=2)
    take = lambda i: np.take_along_axis(v, i[:, :, None, None], axis=2)[:, :, 0, :]
    a3 = any_[..., None]
    rows = np.stack([first + row0[..., 0], last + row0[..., 0]], axis=-1)
    return {"min": np.where(a3, lo.min(axis=2), top).astype(x.dtype), "max": np.where(a3, hi.max(axis=2), 0).astype(x.dtype),
            "argmin": np.where(a3, amin, NO_ROW).astype(np.uint32), "argmax": np.where(a3, amax, NO_ROW).astype(np.uint32),
            "first": np.where(a3, take(first), 0).astype(x.dtype), "last": np.where(a3, take(last), 0).astype(x.dtype),
            "rows": np.where(a3, rows, NO_ROW).astype(np.uint32), "count": s.sum(axis=2).astype(np.uint32)}


def extrema_rows_brute(x, chunk_len, D, mask, W):
    """the same definition, one row at a time"""
    x = np.asarray(x).ravel()
    R = chunk_len // D
    nwin = -(-R // W)
    lens = fm.chunk_counts(x.size, chunk_len)
    top = am.ident_min(x.dtype.itemsize)
    n = len(lens)
    mn = np.full((n, nwin, D), top, np.int64)
    mx = np.zeros((n, nwin, D), np.int64)
    amin = np.full((n, nwin, D), NO_ROW, np.int64)
    amax = np.full((n, nwin, D), NO_ROW, np.int64)
    first = np.zeros((n, nwin, D), np.int64)
    last = np.zeros((n, nwin, D), np.int64)
    rows = np.full((n, nwin, 2), NO_ROW, np.int64)
    cnt = np.zeros((n, nwin), np.int64)
    for c, ne in enumerate(lens):
        for r in range(R):
            if (r + 1) * D > ne or (mask is not None and not (int(mask[c][r >> 3]) >> (r & 7)) & 1):
                continue
            w = r // W
            cnt[c, w] += 1
            if rows[c, w, 0] == NO_ROW:
                rows[c, w, 0] = r
            rows[c, w, 1] = r
            for d in range(D):
                v = int(x[c * chunk_len + r * D + d])
                if amin[c, w, d] == NO_ROW or v < mn[c, w, d]:
                    mn[c, w, d], amin[c, w, d] = v, r
                if amax[c, w, d] == NO_ROW or v > mx[c, w, d]:
                    mx[c, w, d], amax[c, w, d] = v, r
                if rows[c, w, 0] == r:
                    first[c, w, d] = v
                last[c, w, d] = v
    u32 = np.uint32
    return {"min": mn.astype(x.dtype), "max": mx.astype(x.dtype), "argmin": amin.astype(u32), "argmax": amax.astype(u32),
            "first": first.astype(x.dtype), "last": last.astype(x.dtype), "rows": rows.astype(u32), "count": cnt.astype(u32)}


def global_windows(x, chunk_len, D, mask, W):
    """windows over the batch's rows (chunk c holds batch rows [c R, (c + 1) R)): window w covers batch rows [w W, (w + 1) W), w <
    ceil(ceil(n / D) / W).  -> dict: min / max / first / last (x's dtype) [nw, D]; argmin / argmax (int64 batch rows, -1: no selected
    row) [nw, D]; first_row / last_row (int64, -1) and count (int64) [nw]"""
    x = np.asarray(x).ravel()
    R = chunk_len // D
    sel = selected(mask, x.size, chunk_len, D)
    nw = -(-(-(-x.size // D)) // W)
    top = am.ident_min(x.dtype.itemsize)
    out = {"min": np.full((nw, D), top, x.dtype), "max": np.zeros((nw, D), x.dtype), "first": np.zeros((nw, D), x.dtype),
           "last": np.zeros((nw, D), x.dtype), "argmin": np.full((nw, D), -1, np.int64), "argmax": np.full((nw, D), -1, np.int64),
           "first_row": np.full(nw, -1, np.int64), "last_row": np.full(nw, -1, np.int64), "count": np.zeros(nw, np.int64)}
    g = np.concatenate([c * R + np.flatnonzero(sel[c]) for c in range(sel.shape[0])]) if sel.shape[0] else np.zeros(0, np.int64)
    for w in range(nw):
        rows = g[(g >= w * W) & (g < (w + 1) * W)]          # ascending batch rows
        if rows.size == 0:
            continue
        c, r = rows // R, rows % R
        v = np.stack([x[ci * chunk_len + ri * D:ci * chunk_len + (ri + 1) * D] for ci, ri in zip(c, r)])
        out["min"][w], out["max"][w] = v.min(axis=0), v.max(axis=0)
        out["argmin"][w], out["argmax"][w] = rows[v.argmin(axis=0)], rows[v.argmax(axis=0)]
        out["first"][w], out["last"][w] = v[0], v[-1]
        out["first_row"][w], out["last_row"][w], out["count"][w] = rows[0], rows[-1], rows.size
    return out
