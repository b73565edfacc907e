"""The host-side rules ChunkedCodec's row operations share (query_windows, filter_rows, filter_linear, select_rows, aggregate_rows, histogram_rows,
moments_rows, groupby_rows, extrema_rows, segment_rows, float_rows, rolling_rows, project_rows, cumulative_rows, derive_rows, fir_rows, gather_rows), each defined once: a chunk's rows and mask bytes, the mask's shape, the kernel window and the
fold of its results into windows over the batch's rows, the segments' stitching over the chunk seams, the first damaged chunk, float_rows' format and parameters, compress_floats' reciprocal scales, rolling_rows' window rules, counts, mean and scratch size, project_rows' slot table, cumulative_rows' ops, carry, mean and scratch size, the default bin shift, bounds and offsets as tensors, the
linear filter's weights and exactness bound, fir_rows' taps, bound and scratch size, the zone map's classes and the expansion of a pruned filter's results, and the moments' derived values.  Pure functions on torch tensors of any device -- nothing here touches the library, so the CPU tier tests
them (tests/test_rowops_cpu.py)."""
import numpy as np
import torch


def normalise_ops(ops, allowed, what):
    """one name or several -> a tuple of names out of `allowed` (`what`: how the refusal lists them)"""
    ops = (ops,) if isinstance(ops, str) else tuple(ops)
    if not ops or set(ops) - set(allowed):
        raise ValueError(f"ops must be a non-empty subset of {what}, not {ops}")
    return ops


def chunk_rows(chunk_len, ndims, op=None, verb="needs"):
    """-> (R rows a chunk slot, MB mask bytes a chunk slot).  op: the operation that needs whole rows (None: a partial last row counts
    as a row of the slot)"""
    if op is not None and chunk_len % ndims:
        raise ValueError(f"{op} {verb} chunk_len % ndims == 0 ({chunk_len} % {ndims}): rows must not straddle chunks")
    R = -(-chunk_len // ndims)
    return R, -(-R // 8)


def check_mask(mask, n, MB, device):
    """a row mask in filter_rows' layout, n x MB bytes -> the same, contiguous"""
    if not torch.is_tensor(mask) or mask.dtype != torch.uint8 or mask.device != device or mask.numel() != n * MB:
        raise ValueError(f"mask must be a uint8 tensor of {n} x {MB} bytes on {device}")
    return mask.contiguous()


def plan_windows(R, window_rows, per_chunk):
    """The window the kernel is asked for -> (kw, fold, nwin): kw rows a kernel window, nwin = ceil(R / kw) of them a chunk, and `fold`
    consecutive chunks to a window of window_rows batch rows (fold_windows).  window_rows=None: one window a chunk.
    per_chunk=True: window_rows as it is.  Otherwise R must be a multiple of window_rows (the chunk's windows are the batch's) or a divisor
    of it (one window a chunk -- any multiple of 8 that holds R rows -- and window_rows / R chunks fold)."""
    r8 = -(-R // 8) * 8
    W = R if window_rows is None else int(window_rows)
    if W < 1:
        raise ValueError("window_rows must be positive")
    if per_chunk:
        kw, fold = r8 if window_rows is None else W, 1
    elif W % R == 0:
        kw, fold = r8, W // R
    elif R % W == 0:
        kw, fold = W, 1
    else:
        raise ValueError(f"global windows need chunk rows {R} to be a multiple or a divisor of window_rows {W}: use per_chunk=True")
    return kw, fold, -(-R // kw)


def fold_windows(res, n, nwin, D, W, fold, total_len, esz, dtype):
    """The kernel's per-chunk windows {op: [n, nwin, D]}, "count": [n, nwin] -> windows of W rows over the batch's rows {op: [nw, D]},
    "count": [nw], nw = ceil(ceil(total_len / D) / W).  fold == 1: chunk c holds batch rows [c R, (c + 1) R), so its windows are the
    batch's.  fold > 1: one window a chunk, `fold` consecutive chunks a window; the chunks the last window lacks hold the identities (min
    all ones, max 0, sums 0).  min / max reduce as int32: torch's uint16 lacks most reductions."""
    nw = -(-(-(-total_len // D)) // W)
    out = {}
    for k, v in res.items():
        tail = tuple(v.shape[2:])                           # (D,), or () for "count"
        if fold == 1:
            out[k] = v.reshape((n * nwin,) + tail)[:nw]
            continue
        v = v.reshape((n,) + tail)
        if k in ("min", "max"):
            v = v.to(torch.int32)
        ident = (1 << (8 * esz)) - 1 if k == "min" else 0
        v = torch.cat([v, v.new_full((nw * fold - n,) + tail, ident)]).reshape((nw, fold) + tail)
        out[k] = v.amin(dim=1).to(dtype) if k == "min" else v.amax(dim=1).to(dtype) if k == "max" else v.sum(dim=1)
    return out


def fold_extrema(res, n, nwin, D, W, fold, total_len, esz, dtype):
    """extrema_rows' per-chunk windows -> windows of W rows over the batch's rows, as fold_windows does for the aggregates.  res: "min",
    "max", "first", "last": [n, nwin, D] of `dtype`; "argmin", "argmax": int64 [n, nwin, D] and "first_row", "last_row": int64 [n, nwin] --
    BATCH rows, -1 where the window has no selected row; "count": int64 [n, nwin]; any subset, but "argmin" needs "min", "argmax" needs
    "max" and "first" / "last" need "first_row" / "last_row".  fold == 1: the chunks' windows are the batch's.  fold > 1: one window a
    chunk, `fold` consecutive chunks a window: min / argmin come from the FIRST chunk that holds the window's minimum in a selected row
    (chunks lie in batch row order, so that is the first occurrence), max / argmax likewise; first / first_row from the first chunk with
    a selected row, last / last_row from the last one; the chunks the last window lacks hold the identities (min all ones, max 0,
    first = last = 0, rows -1, count 0)."""
    nw = -(-(-(-total_len // D)) // W)
    if fold == 1:
        return {k: v.reshape((n * nwin,) + tuple(v.shape[2:]))[:nw] for k, v in res.items()}
    ident = {"min": (1 << (8 * esz)) - 1, "max": 0, "first": 0, "last": 0, "count": 0}
    g = {}
    for k, v in res.items():
        tail = tuple(v.shape[2:])
        v = v.reshape((n,) + tail)
        if v.dtype == dtype:
            v = v.to(torch.int32)                           # torch's uint16 lacks most reductions
        g[k] = torch.cat([v, v.new_full((nw * fold - n,) + tail, ident.get(k, -1))]).reshape((nw, fold) + tail)
    out = {}

    def pick(v, ok, last=False):
        """v[w, j] at the first (last) j along dim 1 where ok[w, j]; -> (picked, found)"""
        j = torch.arange(fold, device=ok.device).reshape((1, fold) + (1,) * (ok.dim() - 2))
        key = torch.where(ok, j, -1).amax(dim=1) if last else torch.where(ok, j, fold).amin(dim=1)
        found = key >= 0 if last else key < fold
        return v.gather(1, key.clamp(0, fold - 1).unsqueeze(1)).squeeze(1), found

    for val, arg, red in (("min", "argmin", torch.amin), ("max", "argmax", torch.amax)):
        if val not in g:
            continue
        best = red(g[val], dim=1)
        out[val] = best.to(dtype)
        if arg in g:
            a, found = pick(g[arg], (g[val] == best.unsqueeze(1)) & (g[arg] >= 0))
            out[arg] = torch.where(found, a, -1)
    for val, row, last in (("first", "first_row", False), ("last", "last_row", True)):
        if row not in g:
            continue
        ok = g[row] >= 0
        r, found = pick(g[row], ok, last)
        out[row] = torch.where(found, r, -1)
        if val in g:
            v, found = pick(g[val], ok.unsqueeze(-1).expand_as(g[val]), last)
            out[val] = torch.where(found, v, 0).to(dtype)
    if "count" in g:
        out["count"] = g["count"].sum(dim=1)
    return out


SEGMENT_MODES = ("runs", "splits")


def fold_segments(res, mask, R, mode, min_rows, dtype):
    """segment_rows' chunk-relative segments, stitched over the chunk seams on batch rows: what the segment model yields for the batch
    taken as ONE chunk.  res: "start", "rows": int64 [S] -- a segment's first batch row and its length, in ascending batch row order (the
    order of the places when the bases are the counts' prefix sum) -- and any of "min", "max": [S, D] of `dtype`, "sum": int64 [S, D].
    mask: the call's mask, uint8 [nchunks, MB]; R: rows of a chunk slot; mode: "runs" / "splits".
    Segment p continues p - 1 iff it starts where p - 1 ends and that row is a chunk's row 0 -- and, under "splits", bit 0 of that chunk's
    mask is clear (a set bit opens a new segment there whatever lies in front).  Continued segments combine by min of mins, max of
    maxes, sums and rows added; then segments shorter than min_rows are dropped.  -> the same keys, [S'] / [S', D]."""
    if mode not in SEGMENT_MODES:
        raise ValueError("mode must be 'runs' or 'splits'")
    start, rows = res["start"].to(torch.int64).reshape(-1), res["rows"].to(torch.int64).reshape(-1)
    S = start.numel()
    if S == 0:
        return dict(res)
    cont = torch.zeros(S, dtype=torch.bool, device=start.device)
    cont[1:] = (start[1:] == start[:-1] + rows[:-1]) & (start[1:] % R == 0)
    if mode == "splits":
        bit0 = mask.reshape(-1, -(-R // 8))[start // R, 0] & 1
        cont &= bit0 == 0
    head = ~cont
    gid = torch.cumsum(head.to(torch.int64), 0) - 1         # the stitched segment each chunk-relative one belongs to
    G = int(gid[-1].item()) + 1
    out = {"start": start[head], "rows": torch.zeros(G, dtype=torch.int64, device=start.device).index_add_(0, gid, rows)}
    for k in ("min", "max", "sum"):
        if k not in res:
            continue
        v = res[k]
        D = v.shape[-1]
        idx = gid.reshape(S, 1).expand(S, D)
        if k == "sum":
            out[k] = torch.zeros((G, D), dtype=torch.int64, device=v.device).scatter_add_(0, idx, v.to(torch.int64))
        else:                                               # (as int32: torch's uint16 lacks most reductions)
            out[k] = torch.zeros((G, D), dtype=torch.int32, device=v.device).scatter_reduce_(
                0, idx, v.to(torch.int32), "amin" if k == "min" else "amax", include_self=False)
    keep = out["rows"] >= int(min_rows)
    return {k: v[keep].to(dtype) if k in ("min", "max") else v[keep] for k, v in out.items()}


def first_bad(rets, n):
    """the first of rets[:n] that is negative, or None"""
    bad = (rets[:n] < 0).nonzero()
    return int(bad[0, 0].item()) if bad.numel() else None


def raise_damaged(op, rets, n, error):
    """raise error(code, message) naming the first chunk whose decoder returned a negative code, if there is one"""
    c = first_bad(rets, n)
    if c is not None:
        code = int(rets[c].item())
        raise error(code, f"{op}: chunk {c} is damaged (decoder returned {code})")


def float_format(dtype):
    """float_rows' output dtype -> SPRINTZ_FLOAT_F32 / _F16 / _BF16"""
    fmt = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}.get(dtype)
    if fmt is None:
        raise ValueError(f"dtype must be torch.float32, torch.float16 or torch.bfloat16, not {dtype}")
    return fmt


def float_params(v, ndims, name, device):
    """float_rows' scale / offset: None -> None (the library's all 1 / all 0); a number, a sequence of ndims numbers or a tensor of ndims
    elements -> a contiguous float32 tensor [ndims] on `device`.  Host values must be finite."""
    if v is None:
        return None
    if torch.is_tensor(v):
        if v.numel() != ndims:
            raise ValueError(f"{name} must have {ndims} entries, not {v.numel()}")
        return v.reshape(-1).to(device=device, dtype=torch.float32).contiguous()
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, ndims)
    if a.size != ndims:
        raise ValueError(f"{name} must be a number or have {ndims} entries, not {a.size}")
    with np.errstate(over="ignore"):
        a32 = a.astype(np.float32)
    if not np.all(np.isfinite(a)) or not np.all(np.isfinite(a32)):
        raise ValueError(f"{name} must be finite in float32")
    return torch.from_numpy(a32).to(device)


def quant_params(scale, offset, ndims, device):
    """compress_floats' parameters from float_rows' (scale, offset) -> (inv_scale, offset): contiguous float32 tensors [ndims] on `device`,
    or None where the argument is None (the library's all 1 / all 0).  scale / offset: a number, a sequence of ndims numbers or a tensor
    of ndims elements.  inv_scale = 1 / scale, one float32 division an entry.  A scale that is zero or not finite -- or so small that its
    reciprocal is not finite in float32 -- is a ValueError, as is an offset that is not finite."""
    off = float_params(offset, ndims, "offset", device)
    if off is not None and torch.is_tensor(offset) and not bool(torch.isfinite(off).all()):
        raise ValueError("offset must be finite in float32")
    if scale is None:
        return None, off
    if torch.is_tensor(scale):
        if scale.numel() != ndims:
            raise ValueError(f"scale must have {ndims} entries, not {scale.numel()}")
        s = scale.reshape(-1).to(dtype=torch.float32)
    else:
        a = np.asarray(scale, dtype=np.float64).reshape(-1)
        if a.size == 1:
            a = np.repeat(a, ndims)
        if a.size != ndims:
            raise ValueError(f"scale must be a number or have {ndims} entries, not {a.size}")
        with np.errstate(over="ignore"):
            s = torch.from_numpy(a.astype(np.float32))
    if not bool(torch.isfinite(s).all()) or bool((s == 0).any()):
        raise ValueError("scale must be finite in float32 and not zero")
    inv = torch.ones_like(s) / s
    if not bool(torch.isfinite(inv).all()):
        raise ValueError("1 / scale must be finite in float32")
    return inv.to(device).contiguous(), off


ROLLING_OPS = ("min", "max", "sum", "mean")


def rolling_window(window_rows, R, esz):
    """rolling_rows' window -> W as an int: a multiple of 8 with 8 <= W <= R rows of a chunk (one predecessor chunk suffices at a seam) and
    W * (2^(8 esz) - 1) < 2^31 (the sum is an int32).  The bound by the kernel's LDS is the library's to refuse: it depends on the lane mapping."""
    W = int(window_rows)
    if W != window_rows or W < 8 or W % 8:
        raise ValueError(f"window_rows must be a multiple of 8, at least 8, not {window_rows}")
    if W > R:
        raise ValueError(f"window_rows {W} exceeds the {R} rows of a chunk: a window may reach into one chunk in front, not two")
    if W * ((1 << (8 * esz)) - 1) >= 1 << 31:
        raise ValueError(f"window_rows {W} x the largest {8 * esz}-bit element does not fit the int32 sum")
    return W


def rolling_counts(G, W, device=None):
    """the rows in the trailing window of W rows that ends at batch row g, clipped at row 0: min(g + 1, W), int32 [G]"""
    return torch.clamp(torch.arange(1, G + 1, dtype=torch.int64, device=device), max=W).to(torch.int32)


def rolling_mean(total, counts):
    """rolling sums int32 [G, D] and their rows' counts [G] -> the means, float32 [G, D]: one float32 divide of the converted integers"""
    return total.to(torch.float32) / counts.to(torch.float32).unsqueeze(1)


def rolling_tmp_bytes(nchunks, W, ndims, esz):
    """the seam scratch rolling_rows needs with more than one chunk (include/sprintz_mi355x.h: d_tmp), a multiple of 16 bytes a chunk"""
    return nchunks * ((16 + (W - 1) * ndims * esz + 15) & ~15) if nchunks > 1 else 0


def project_slots(columns, ndims, device=None):
    """project_rows' columns -> the slot table the library reads, int32 [ndims] on `device`: slots[c_j] = j, -1 for a column that is not
    wanted.  columns: K >= 1 distinct ints in 0 .. ndims - 1, in any order (a permutation, and the identity, are legal)."""
    cols = columns.tolist() if torch.is_tensor(columns) or isinstance(columns, np.ndarray) else list(columns)
    if not cols:
        raise ValueError("columns must name at least one column")
    slots = [-1] * ndims
    for j, c in enumerate(cols):
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
            raise ValueError(f"columns must be ints, not {c!r}")
        if not 0 <= c < ndims:
            raise ValueError(f"column {c} is outside 0 .. {ndims - 1}")
        if slots[c] >= 0:
            raise ValueError(f"column {c} is named twice")
        slots[c] = j
    return torch.tensor(slots, dtype=torch.int32, device=device)


CUMULATIVE_OPS = ("min", "max", "sum", "mean")


class CumulativeCarry:
    """what one cumulative_rows call hands to the next: `table`, int64 [3, ndims] -- the library's carry, a min row, a max row and a sum row (the
    bits of its uint64) -- and `rows`, the batch rows behind it, which the expanding mean divides by"""

    def __init__(self, table, rows=0):
        self.table = table
        self.rows = int(rows)


def cumulative_carry(ndims, esz, device=None):
    """the carry in front of a stream's first batch: the identities -- all ones of the element type, 0 and 0 -- and no row"""
    table = torch.zeros((3, ndims), dtype=torch.int64, device=device)
    table[0] = (1 << (8 * esz)) - 1
    return CumulativeCarry(table, 0)


def check_carry(carry, ndims, device):
    """a carry as cumulative_rows returned it, for a codec of ndims columns on `device` -> the same"""
    t = getattr(carry, "table", None)
    if not torch.is_tensor(t) or t.dtype != torch.int64 or t.device != device or tuple(t.shape) != (3, ndims) or not t.is_contiguous():
        raise ValueError(f"carry must be what cumulative_rows returned for {ndims} columns on {device}")
    return carry


def cumulative_mean(total, rows_before=0):
    """cumulative sums int64 [G, D], behind rows_before rows of earlier batches -> the expanding means, float64 [G, D]: the converted sum
    over the rows so far, rows_before + g + 1"""
    G = total.shape[0]
    n = torch.arange(rows_before + 1, rows_before + G + 1, dtype=torch.float64, device=total.device)
    return total.to(torch.float64) / n.unsqueeze(1)


def cumulative_tmp_bytes(nchunks, ndims):
    """the scratch cumulative_rows needs with more than one chunk (sprintz_mi355x_cumulative_tmp_bytes; geom.h: cum_tmp_layout): the chunks'
    entering states, the totals pass' return values, and the chunks' sums, minima and maxima, each region rounded up to 16 bytes"""
    if nchunks <= 1:
        return 0
    nd = nchunks * ndims

    def r16(x):
        return (x + 15) & ~15

    return r16(nd * 24) + r16(nchunks * 8) + r16(nd * 8) + 2 * r16(nd * 2)


def default_shift(W, nbins):
    """the shift that makes nbins bins cover the range of W-bit elements, W - ceil(log2(nbins)) (one bin: the largest there is, W - 1)"""
    return min(max(W - max(nbins - 1, 0).bit_length(), 0), W - 1)


def _entries(v, ndims, name):
    """a scalar (None is one) or a sequence -> a list of ndims entries"""
    vals = [v] * ndims if v is None or np.isscalar(v) else list(v)
    if len(vals) != ndims:
        raise ValueError(f"{name} must be a scalar or have {ndims} entries, not {len(vals)}")
    return vals


def elem_tensor(v, ndims, esz, dtype, device, name, open_end=None):
    """a scalar, a sequence of ndims entries or a tensor of ndims integers -> a contiguous tensor [ndims] of `dtype` on `device`.
    open_end: what a None entry stands for -- v is a bound then, which is compared as it is: entries may be None, and a tensor must be of
    `dtype`.  Without it v is an offset: a tensor of another dtype is taken modulo 2^W."""
    W = 8 * esz
    bound = open_end is not None
    if torch.is_tensor(v):
        if v.numel() != ndims or (bound and v.dtype != dtype):
            raise ValueError(f"{name} must hold {ndims} entries" + (f" of {dtype}" if bound else ""))
        v = v.to(device).reshape(-1)
        if v.dtype == dtype:
            return v.contiguous()
        half = 1 << (W - 1)                                 # through the signed type of the same width: torch's uint16 lacks arithmetic
        s = ((v.to(torch.int64) + half) % (1 << W)) - half
        return s.to(torch.int8 if esz == 1 else torch.int16).view(dtype).contiguous()
    vals = [open_end if bound and e is None else e for e in _entries(v, ndims, name)]
    if any(not 0 <= int(e) < (1 << W) for e in vals):
        raise ValueError(f"{name} entries must be in 0..{(1 << W) - 1}")
    a = np.array([int(e) for e in vals], np.uint8 if esz == 1 else np.uint16)
    return torch.from_numpy(a.view(np.int8 if esz == 1 else np.int16)).to(device).view(dtype)


def filter_bounds(lo, hi, mode, ndims, esz, dtype, device):
    """filter_rows' lo / hi -- a scalar, a sequence of ndims entries (None: an open end) or a tensor of `dtype` -- as two contiguous tensors
    [ndims].  A column with neither bound is unconstrained: it always matches under "all" and never -- an empty interval -- under "any"."""
    top = (1 << (8 * esz)) - 1
    if mode == "any" and not torch.is_tensor(lo) and not torch.is_tensor(hi):
        lo, hi = _entries(lo, ndims, "lo"), _entries(hi, ndims, "hi")
        for d in range(ndims):
            if lo[d] is None and hi[d] is None:
                lo[d], hi[d] = top, 0
    return elem_tensor(lo, ndims, esz, dtype, device, "lo", 0), elem_tensor(hi, ndims, esz, dtype, device, "hi", top)


INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def _weights(v, ndims, name):
    """a scalar (every column), a sequence of ndims entries, a dict {column: weight} (the others 0) or a tensor of ndims integers ->
    a list of ndims Python ints"""
    if torch.is_tensor(v):
        if v.numel() != ndims or v.dtype.is_floating_point or v.dtype == torch.bool:
            raise ValueError(f"{name} must hold {ndims} integers")
        return [int(e) for e in v.reshape(-1).cpu().tolist()]
    if isinstance(v, dict):
        vals = [0] * ndims
        for d, e in v.items():
            if not 0 <= int(d) < ndims:
                raise ValueError(f"{name}: column {d} outside 0..{ndims - 1}")
            vals[int(d)] = int(e)
        return vals
    return [int(e) for e in _entries(v, ndims, name)]


def linear_bound(w, u, bias, esz, what="the linear form"):
    """B = |bias| + (2^W - 1) sum_d (|w[d]| + |u[d]|) of one form (lists of ints; u None: no lag term): below 2^31 the kernels' wrapping 32-bit
    sum is the exact integer, so a form that can reach 2^31 is a ValueError -- filter_linear's rule and derive_rows', stated once"""
    B = abs(bias) + ((1 << (8 * esz)) - 1) * (sum(abs(e) for e in w) + sum(abs(e) for e in u or ()))
    if B >= 1 << 31:
        raise ValueError(f"{what} can reach {B} in magnitude: |bias| + (2^{8 * esz} - 1) sum(|w| + |u|) must stay below 2^31, "
                         "or the 32-bit sum wraps")
    return B


def linear_terms(weights, lag_weights, bias, lo, hi, ndims, esz, device):
    """filter_linear's arguments -> (w, u, bias, lo, hi): w and u contiguous int32 tensors [ndims] on `device` (u None where
    lag_weights is None: no lag term), bias / lo / hi Python ints that fit int32.  weights / lag_weights: a scalar (every column), a
    sequence of ndims entries, a dict {column: weight} or a tensor of ndims integers.  lo / hi of None are the open ends of int32.
    The kernel's sum wraps modulo 2^32; it is the exact integer wherever
        B = |bias| + (2^W - 1) sum_d (|w[d]| + |u[d]|) < 2^31,     W = 8 esz,
    so a form with B >= 2^31 is refused, as is a bound that does not fit int32."""
    w = _weights(weights, ndims, "weights")
    u = None if lag_weights is None else _weights(lag_weights, ndims, "lag_weights")
    bias = int(bias)
    lo = INT32_MIN if lo is None else int(lo)
    hi = INT32_MAX if hi is None else int(hi)
    for name, v in (("lo", lo), ("hi", hi)):
        if not INT32_MIN <= v <= INT32_MAX:
            raise ValueError(f"{name} = {v} does not fit int32")
    linear_bound(w, u, bias, esz)
    as_t = lambda vals: torch.from_numpy(np.array(vals, np.int32)).to(device)      # noqa: E731
    return as_t(w), None if u is None else as_t(u), bias, lo, hi


DERIVE_MAX_FORMS = 16


def derive_forms(forms, lag_forms, bias, ndims, esz, device):
    """derive_rows' arguments -> (w, u, bias): w and u contiguous int32 tensors [K, ndims] on `device` (u None where lag_forms is None: no lag
    term) and bias an int32 tensor [K].  forms / lag_forms: an integer tensor [K, ndims], or a sequence of K entries, each as filter_linear takes
    its weights -- a scalar (every column), a sequence of ndims entries, a dict {column: weight} or a tensor of ndims integers.  bias: a scalar
    (every form) or K entries.  1 <= K <= 16, and lag_forms, where given, has K entries too.  Every form is held to linear_terms' bound
    (linear_bound): one that can reach 2^31 in magnitude is refused, by its number."""
    def rows(v, name):
        if torch.is_tensor(v):
            if v.dim() != 2 or v.shape[1] != ndims or v.dtype.is_floating_point or v.dtype == torch.bool:
                raise ValueError(f"{name} must be an integer tensor [K, {ndims}]")
            return [[int(e) for e in r] for r in v.cpu().tolist()]
        if isinstance(v, dict) or np.isscalar(v):
            raise ValueError(f"{name} must be a sequence of forms (K entries), not one form")
        return [_weights(f, ndims, f"{name}[{k}]") for k, f in enumerate(v)]
    w = rows(forms, "forms")
    K = len(w)
    if not 1 <= K <= DERIVE_MAX_FORMS:
        raise ValueError(f"derive_rows takes 1 .. {DERIVE_MAX_FORMS} forms, not {K}")
    u = None if lag_forms is None else rows(lag_forms, "lag_forms")
    if u is not None and len(u) != K:
        raise ValueError(f"lag_forms must have as many entries as forms ({K}), not {len(u)}")
    b = [int(e) for e in _entries(bias, K, "bias")]
    for k in range(K):
        linear_bound(w[k], None if u is None else u[k], b[k], esz, f"form {k}")
    as_t = lambda vals: torch.from_numpy(np.array(vals, np.int32).reshape(K, -1)).to(device)      # noqa: E731
    return as_t(w), None if u is None else as_t(u), as_t(b).reshape(K)


FIR_MAX_TAPS = 256


def fir_taps(taps, bias, ndims, esz, device):
    """fir_rows' arguments -> (taps, bias): taps a contiguous int32 tensor [T, ndims] on `device`, taps[0] weighing the row itself, and bias an
    int32 tensor [ndims].  taps: a 1-D sequence (or tensor) of T integers, shared by all columns, or [T, ndims] -- a sequence of T rows of ndims
    integers, or an integer tensor.  bias: a scalar (every column) or ndims entries.  1 <= T <= 256.  Every column's filter is held to
    linear_bound: |bias[d]| + (2^W - 1) sum_j |taps[j][d]| must stay below 2^31, and one that can reach it is refused, by its column."""
    if torch.is_tensor(taps):
        if taps.dtype.is_floating_point or taps.dtype == torch.bool or taps.dim() not in (1, 2) or (taps.dim() == 2 and taps.shape[1] != ndims):
            raise ValueError(f"taps must be an integer tensor [T] or [T, {ndims}]")
        rows = taps.cpu().tolist()
    elif isinstance(taps, dict) or np.isscalar(taps) or taps is None:
        raise ValueError("taps must be a sequence of T entries, not one entry")
    else:
        rows = list(taps)
    T = len(rows)
    if not 1 <= T <= FIR_MAX_TAPS:
        raise ValueError(f"fir_rows takes 1 .. {FIR_MAX_TAPS} taps, not {T}")
    if all(np.isscalar(r) for r in rows):
        rows = [[r] * ndims for r in rows]
    t = []
    for j, r in enumerate(rows):
        if np.isscalar(r) or len(r) != ndims:
            raise ValueError(f"taps[{j}] must have {ndims} entries: taps is [T] (shared by all columns) or [T, {ndims}]")
        if any(isinstance(e, (float, np.floating)) for e in r):
            raise ValueError(f"taps[{j}] must hold integers")
        t.append([int(e) for e in r])
    b = [int(e) for e in _entries(bias, ndims, "bias")]
    for d in range(ndims):
        linear_bound([t[j][d] for j in range(T)], None, b[d], esz, f"column {d}'s filter")
    return torch.from_numpy(np.array(t, np.int32).reshape(T, ndims)).to(device), torch.from_numpy(np.array(b, np.int32)).to(device)


def fir_tmp_bytes(nchunks, T, ndims, esz):
    """the seam scratch fir_rows needs with more than one tap (include/sprintz_mi355x.h: d_tmp; fir_tmp_stride in geom.h), a multiple of 16 bytes a chunk"""
    return nchunks * ((16 + 2 * (T - 1) * ndims * esz + 15) & ~15) if T > 1 else 0


def shift_taps(k):
    """shift_rows' taps: a unit tap at lag k"""
    k = int(k)
    if not 0 <= k < FIR_MAX_TAPS:
        raise ValueError(f"k must be in 0 .. {FIR_MAX_TAPS - 1}, not {k}")
    return [0] * k + [1]


def lag_diff_taps(periods):
    """lag_diff_rows' taps: +1 at lag 0 and -1 at lag `periods`"""
    p = int(periods)
    if not 1 <= p < FIR_MAX_TAPS:
        raise ValueError(f"periods must be in 1 .. {FIR_MAX_TAPS - 1}, not {periods}")
    return [1] + [0] * (p - 1) + [-1]


ZONE_NONE, ZONE_ALL, ZONE_DECODE = 0, 1, 2
ZONE_SPAN_LIMIT = 0xF0000000


def check_zones(zones, nchunks, ndims, general_layout, quirk):
    """a ZoneMap against the call it is to prune: the batch's chunks and columns, and the layout flag and SPRINTZ_OPT_REF_DECODER_QUIRK
    state it was built under -- a map built under another decodes other values, so it is refused"""
    if tuple(zones.min.shape) != (nchunks, ndims) or tuple(zones.max.shape) != (nchunks, ndims) or zones.len.numel() != nchunks:
        raise ValueError(f"zones describe {zones.len.numel()} chunks of {tuple(zones.min.shape)[-1:]} columns, the batch has {nchunks} of {ndims}")
    if bool(zones.general_layout) != bool(general_layout):
        raise ValueError(f"zones were built with general_layout={bool(zones.general_layout)}, the call has general_layout={bool(general_layout)}")
    if int(zones.quirk) != int(quirk):
        raise ValueError(f"zones were built with SPRINTZ_OPT_REF_DECODER_QUIRK = {int(zones.quirk)}, the process now decodes under {int(quirk)}")


def zone_rows(zlen, chunk_len, ndims):
    """existing rows of chunks whose decoder returned zlen >= 0 elements: int64, like zlen"""
    return torch.clamp(zlen.to(torch.int64) // ndims, max=chunk_len // ndims)


def _zone_finish(verdict, zlen, chunk_len, ndims, span):
    """what the element count and the container's span decide, over the bounds' verdict"""
    zlen = zlen.to(torch.int64).reshape(-1)
    cls = torch.where(zone_rows(zlen, chunk_len, ndims) == 0, ZONE_NONE, verdict)
    if span >= ZONE_SPAN_LIMIT:                             # the 4 GiB rule: the container is not pruned
        cls = torch.full_like(cls, ZONE_DECODE)
    return torch.where(zlen < 0, ZONE_DECODE, cls).to(torch.uint8)


def zone_classify_box(zmin, zmax, zlen, lo, hi, mode, chunk_len, ndims, span=0):
    """The host reference of sprintz_mi355x_zone_prune_box's classes (include/sprintz_mi355x.h).  zmin / zmax: [n, ndims], zlen: [n], lo / hi:
    [ndims], integer tensors of any dtype; mode "all" / "any"; span = offsets[n] - offsets[0].  -> uint8 [n] of ZONE_NONE / _ALL / _DECODE"""
    zmin, zmax = zmin.to(torch.int64).reshape(-1, ndims), zmax.to(torch.int64).reshape(-1, ndims)
    lo, hi = lo.to(torch.int64).reshape(1, ndims), hi.to(torch.int64).reshape(1, ndims)
    disjoint = (lo > hi) | (zmax < lo) | (zmin > hi)
    inside = (lo <= zmin) & (zmax <= hi)
    none, every, decode = (torch.full((zmin.shape[0],), k, dtype=torch.int64, device=zmin.device) for k in (ZONE_NONE, ZONE_ALL, ZONE_DECODE))
    if mode == "all":
        verdict = torch.where(disjoint.any(dim=1), none, torch.where(inside.all(dim=1), every, decode))
    elif mode == "any":
        verdict = torch.where(inside.any(dim=1), every, torch.where(disjoint.all(dim=1), none, decode))
    else:
        raise ValueError("mode must be 'all' or 'any'")
    return _zone_finish(verdict, zlen, chunk_len, ndims, span)


def zone_classify_linear(zmin, zmax, zlen, weights, bias, lo, hi, chunk_len, ndims, span=0):
    """The host reference of sprintz_mi355x_zone_prune_linear's classes: the form's range over a chunk in int64, left to the decoder where
    it leaves int32.  weights: [ndims] integers; bias, lo, hi: Python ints.  -> uint8 [n]"""
    zmin, zmax = zmin.to(torch.int64).reshape(-1, ndims), zmax.to(torch.int64).reshape(-1, ndims)
    w = weights.to(torch.int64).reshape(1, ndims)
    smin = int(bias) + torch.where(w >= 0, w * zmin, w * zmax).sum(dim=1)
    smax = int(bias) + torch.where(w >= 0, w * zmax, w * zmin).sum(dim=1)
    lo, hi = int(lo), int(hi)
    none, every, decode = (torch.full_like(smin, k) for k in (ZONE_NONE, ZONE_ALL, ZONE_DECODE))
    verdict = torch.where((smax < lo) | (smin > hi), none, torch.where((smin >= lo) & (smax <= hi), every, decode))
    if lo > hi:
        verdict = none
    verdict = torch.where((smin < INT32_MIN) | (smax > INT32_MAX), decode, verdict)
    return _zone_finish(verdict, zlen, chunk_len, ndims, span)


def zone_expand(cls, zlen, cmask, ccounts, crets, chunk_len, ndims):
    """The host reference of sprintz_mi355x_zone_expand: a filter's compact results over the ZONE_DECODE chunks, in batch order -- cmask
    uint8 [n', MB], ccounts [n'], crets [n'] -- into filter_rows' layout -> (mask uint8 [n, MB], counts int64 [n], rets int64 [n]).  A
    ZONE_NONE chunk matches nowhere; a ZONE_ALL chunk has the bits of its existing rows set and the padding bits of its last byte 0; a chunk with zlen < 0 keeps zlen as its ret."""
    R, MB = chunk_rows(chunk_len, ndims)
    cls, zlen = cls.reshape(-1), zlen.to(torch.int64).reshape(-1)
    n = cls.numel()
    dec = cls == ZONE_DECODE
    rows = torch.where(cls == ZONE_ALL, zone_rows(zlen, chunk_len, ndims), 0)
    bit = torch.arange(MB * 8, device=cls.device).reshape(1, MB, 8)
    mask = ((bit < rows.reshape(n, 1, 1)).to(torch.int64) << torch.arange(8, device=cls.device)).sum(dim=2).to(torch.uint8)
    counts, rets = rows.clone(), zlen.clone()
    mask[dec] = cmask.reshape(-1, MB).to(torch.uint8)
    counts[dec] = ccounts.reshape(-1).to(torch.int64)
    rets[dec] = crets.reshape(-1).to(torch.int64)
    rets = torch.where(zlen < 0, zlen, rets)                # a chunk the map found damaged keeps the map's code, whatever the decoder made of it
    return mask, counts, rets


def derive_moments(out, ops, ref, ddof):
    """The derived moments among `ops` -- "mean", "var", "std", "cov", "corr" -- of the integer sums out["count"] [...], out["sum"],
    out["sumsq"], out["cross"] [..., D] (int64; only what the ops need), as float64 [..., D].  NaN where n == 0 or n <= ddof, and corr
    also where either variance is 0.

    They are NOT formed as n Q - S^2 in float64: that difference reaches 2^94 and cancels.  With the integer pivot m = S // n and
    r = S - n m (0 <= r < n),
        C = Q - 2 m S + n m^2 = sum (x - m)^2
    in wrapping int64 arithmetic: intermediates may wrap, but two's-complement arithmetic is exact modulo 2^64 and 0 <= C <= Q < 2^63,
    so C is exact.  Then n var = C - r^2 / n, i.e.
        var = C / (n - ddof) - (r / n) (r / (n - ddof))
    in float64: the second term is at most 1 and the first is never smaller than the result, so nothing cancels badly.  Likewise with
    two pivots, Cxy = P - m_x S_y - m_y S_x + n m_x m_y = sum (x - m_x)(y - m_y) (|Cxy| < 2^62: exact as a signed int64) and
        cov = Cxy / (n - ddof) - (r_x / n) (r_y / (n - ddof)),     corr = cov_0 / sqrt(var_0(x) var_0(y))   (ddof = 0 throughout).
    A variance is 0 exactly where C == 0."""
    f64 = torch.float64
    cnt = out["count"].unsqueeze(-1)                        # [..., 1]
    n1 = cnt.clamp(min=1)
    nf = cnt.to(f64)
    nd = (cnt - ddof).to(f64)
    S = out["sum"]
    m = S // n1                                             # the integer pivot, and what it leaves: 0 <= r < n
    r = S - cnt * m
    nan = torch.full((), float("nan"), dtype=f64, device=cnt.device)
    der = {}

    def centred2():                                         # C = sum (x - m)^2, exact (see above)
        return out["sumsq"] - 2 * m * S + cnt * m * m

    def centred_xy():                                       # Cxy = sum (x - m_x)(x_ref - m_ref), exact
        j = int(ref)
        return out["cross"] - m * S[..., j:j + 1] - m[..., j:j + 1] * S + cnt * m * m[..., j:j + 1]

    if "mean" in ops:
        der["mean"] = torch.where(cnt > 0, S.to(f64) / nf, nan)
    if set(ops) & {"var", "std"}:
        var = centred2().to(f64) / nd - (r.to(f64) / nf) * (r.to(f64) / nd)
        var = torch.where(cnt > ddof, var, nan)
        if "var" in ops:
            der["var"] = var
        if "std" in ops:
            der["std"] = var.clamp(min=0.0).sqrt()          # (a variance below its own rounding error may come out as -1e-16)
    if "cov" in ops:
        j = int(ref)
        rf = r.to(f64)
        cov = centred_xy().to(f64) / nd - (rf / nf) * (rf[..., j:j + 1] / nd)
        der["cov"] = torch.where(cnt > ddof, cov, nan)
    if "corr" in ops:
        j = int(ref)
        rf = r.to(f64)
        C = centred2()
        v0 = C.to(f64) / nf - (rf / nf) * (rf / nf)
        c0 = centred_xy().to(f64) / nf - (rf / nf) * (rf[..., j:j + 1] / nf)
        ok = (cnt > 0) & (C != 0) & (C[..., j:j + 1] != 0)
        der["corr"] = torch.where(ok, c0 / (v0 * v0[..., j:j + 1]).sqrt(), nan)
    return der
