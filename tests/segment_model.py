"""numpy model of segment rows (sprintz_mi355x_segment_count / sprintz_mi355x_segment_rows, include/sprintz_mi355x.h), applied to the
ORIGINAL input -- decode is lossless and pinned elsewhere -- and a one-row-at-a-time brute force of the same definition.

chunk_len % D == 0; R = chunk_len // D rows a chunk slot, MB = ceil(R / 8) mask bytes a chunk slot.  rows_c is the number of whole rows
chunk c holds; b[r] is bit r & 7 of mask[c, r >> 3] for r < rows_c and 0 for every other r.  Under RUNS a row is a member iff b[r] and
a start iff b[r] and not b[r - 1] (b[-1] = 0); under SPLITS every row is a member and a start iff b[r] or r == 0.  Segment i of a chunk
is its i-th start s_i and covers [s_i, e_i), e_i the first row behind s_i that is not a member or is a start, else rows_c."""
import numpy as np

import filter_model as fm

RUNS, SPLITS = 0, 1
MIN, MAX, SUM, ROWS, START = 1, 2, 4, 8, 16


def mask_bits(mask, R):
    """uint8 [nchunks, MB] -> bool [nchunks, R]"""
    return np.unpackbits(np.asarray(mask, np.uint8), axis=1, bitorder="little")[:, :R].astype(bool)


def pack_bits(bits):
    """bool [nchunks, R] -> uint8 [nchunks, MB], padding bits 0"""
    return np.packbits(np.asarray(bits, bool), axis=1, bitorder="little")


def chunk_rows(n, chunk_len, D):
    """the whole rows of every chunk of a flat array of n elements"""
    return [ne // D for ne in fm.chunk_counts(n, chunk_len)]


def edges(b, mode):
    """b: bool [rows] -- the bits of the rows that exist.  -> (s, e): int64 arrays, segment i covers rows [s[i], e[i])"""
    b = np.asarray(b, bool)
    rows = b.size
    if rows == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if mode == SPLITS:
        st = b.copy()
        st[0] = True
        s = np.flatnonzero(st)
        return s, np.append(s[1:], rows)
    prev = np.concatenate(([False], b[:-1]))
    nxt = np.concatenate((b[1:], [False]))
    return np.flatnonzero(b & ~prev), np.flatnonzero(b & ~nxt) + 1


def reduce_segments(v, s, e):
    """v: [rows, D]; -> min / max (v's dtype), sum (uint64) [S, D] over rows [s[i], e[i])"""
    D = v.shape[1]
    if s.size == 0:
        return {"min": np.zeros((0, D), v.dtype), "max": np.zeros((0, D), v.dtype), "sum": np.zeros((0, D), np.uint64)}
    pad = np.concatenate((v, np.zeros((1, D), v.dtype)))    # (an end may be the row behind the last one)
    idx = np.stack((s, e), axis=1).ravel()
    return {"min": np.minimum.reduceat(pad, idx)[::2], "max": np.maximum.reduceat(pad, idx)[::2],
            "sum": np.add.reduceat(pad.astype(np.uint64), idx)[::2]}


def segment_count(mask, chunk_len, D, mode, lens=None):
    """mask: uint8 [nchunks, MB]; lens: element counts a chunk (negative: no row) or None: R rows in every chunk.  -> uint32 [nchunks]"""
    R = chunk_len // D
    bits = mask_bits(mask, R)
    out = np.zeros(bits.shape[0], np.uint32)
    for c in range(bits.shape[0]):
        rows = R if lens is None else min(R, max(int(lens[c]), 0) // D)
        out[c] = edges(bits[c, :rows], mode)[0].size
    return out


def segment_rows(x, chunk_len, D, mask, mode):
    """x: the flat original array; mask: uint8 [nchunks, MB].  -> dict, the chunks' segments in chunk order: "counts" uint32 [nchunks],
    "chunk" int64 [S], "start" uint64 [S] (batch row c * R + s_i), "rows" uint32 [S], "min" / "max" (x's dtype) and "sum" (uint64) [S, D]"""
    assert chunk_len % D == 0
    x = np.asarray(x).ravel()
    R = chunk_len // D
    bits = mask_bits(mask, R)
    parts = {"chunk": [np.zeros(0, np.int64)], "start": [np.zeros(0, np.uint64)], "rows": [np.zeros(0, np.uint32)],      # (a batch may hold no chunk)
             "min": [np.zeros((0, D), x.dtype)], "max": [np.zeros((0, D), x.dtype)], "sum": [np.zeros((0, D), np.uint64)]}
    counts = []
    for c, rows in enumerate(chunk_rows(x.size, chunk_len, D)):
        v = x[c * chunk_len:c * chunk_len + rows * D].reshape(rows, D)
        s, e = edges(bits[c, :rows], mode)
        counts.append(s.size)
        red = reduce_segments(v, s, e)
        parts["chunk"].append(np.full(s.size, c, np.int64))
        parts["start"].append((c * R + s).astype(np.uint64))
        parts["rows"].append((e - s).astype(np.uint32))
        for k in ("min", "max", "sum"):
            parts[k].append(red[k])
    out = {k: np.concatenate(v) for k, v in parts.items()}
    out["counts"] = np.array(counts, np.uint32)
    return out


def batch_bits(mask, n, chunk_len, D):
    """the mask over the batch's rows: bool [whole rows of the batch], chunk c's existing rows at [c R, ...) -- every chunk but the last
    of a flat array is full, so those are the batch's rows in order"""
    R = chunk_len // D
    bits = mask_bits(mask, R)
    return np.concatenate([bits[c, :rows] for c, rows in enumerate(chunk_rows(n, chunk_len, D))] or [np.zeros(0, bool)])


def segment_rows_one_chunk(x, chunk_len, D, mask, mode, min_rows=1):
    """the batch taken as ONE chunk (what ChunkedCodec.segment_rows returns): -> "start", "rows" int64 [S], "min" / "max" (x's dtype),
    "sum" int64 [S, D]; segments shorter than min_rows dropped"""
    x = np.asarray(x).ravel()
    b = batch_bits(mask, x.size, chunk_len, D)
    v = x[:b.size * D].reshape(b.size, D)
    s, e = edges(b, mode)
    keep = (e - s) >= min_rows
    s, e = s[keep], e[keep]
    red = reduce_segments(v, s, e)
    return {"start": s.astype(np.int64), "rows": (e - s).astype(np.int64), "min": red["min"], "max": red["max"], "sum": red["sum"].astype(np.int64)}


def segment_rows_brute(x, chunk_len, D, mask, mode):
    """the same definition as segment_rows, one row at a time"""
    x = np.asarray(x).ravel()
    R = chunk_len // D
    top = (1 << (8 * x.dtype.itemsize)) - 1
    chunk, start, rows, mn, mx, sm, counts = [], [], [], [], [], [], []
    for c, rows_c in enumerate(chunk_rows(x.size, chunk_len, D)):
        bit = lambda r: 0 <= r < rows_c and bool((int(mask[c][r >> 3]) >> (r & 7)) & 1)      # noqa: E731
        nseg, open_ = 0, False
        for r in range(rows_c):
            member = bit(r) if mode == RUNS else True
            is_start = (bit(r) and not bit(r - 1)) if mode == RUNS else (bit(r) or r == 0)
            if open_ and (is_start or not member):
                open_ = False
            if is_start:
                open_ = True
                nseg += 1
                chunk.append(c); start.append(c * R + r); rows.append(0)
                mn.append([top] * D); mx.append([0] * D); sm.append([0] * D)
            if member:
                assert open_
                rows[-1] += 1
                for d in range(D):
                    v = int(x[c * chunk_len + r * D + d])
                    mn[-1][d] = min(mn[-1][d], v)
                    mx[-1][d] = max(mx[-1][d], v)
                    sm[-1][d] += v
        counts.append(nseg)
    S = len(start)
    return {"counts": np.array(counts, np.uint32), "chunk": np.array(chunk, np.int64), "start": np.array(start, np.uint64),
            "rows": np.array(rows, np.uint32), "min": np.array(mn, x.dtype).reshape(S, D), "max": np.array(mx, x.dtype).reshape(S, D),
            "sum": np.array(sm, np.uint64).reshape(S, D)}


def placed(model, bases, capacity, D, dtype, sentinel, pad=0):
    """the five outputs as the call leaves them in buffers of capacity + pad entries pre-filled with the byte `sentinel`: segment i of chunk
    c at bases[c] + i, a place >= capacity dropped.  -> dict of flat arrays: "min" / "max" [(capacity + pad) * D] of dtype, "sum" uint64
    [(capacity + pad) * D], "rows" uint32 [capacity + pad], "start" uint64 [capacity + pad]; and "written": bool [capacity + pad]"""
    n = capacity + pad
    fill = lambda shape, dt: np.frombuffer(bytes([sentinel]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dt).reshape(shape).copy()      # noqa: E731
    out = {"min": fill((n, D), dtype), "max": fill((n, D), dtype), "sum": fill((n, D), np.uint64), "rows": fill((n,), np.uint32),
           "start": fill((n,), np.uint64)}
    written = np.zeros(n, bool)
    first = np.concatenate(([0], np.cumsum(model["counts"].astype(np.int64))))[:-1]
    chunk = model["chunk"]
    place = np.asarray(bases, np.int64)[chunk] + (np.arange(chunk.size) - first[chunk])
    ok = place < capacity
    assert np.unique(place[ok]).size == int(ok.sum()), "the bases make two segments share a place"
    written[place[ok]] = True
    for k in out:
        out[k][place[ok]] = model[k][ok]
    out = {k: v.reshape(-1) for k, v in out.items()}
    out["written"] = written
    return out


def ruler_bits(n):
    """bool [n]: runs of 1 .. 17 set rows with gaps of 1 .. 9 clear rows between them, over and over -- 17 and 9 share no factor with 8, so
    a run's start and its end meet every phase against the 8-row block"""
    out = np.zeros(n, bool)
    r, run, gap = 0, 1, 1
    while r < n:
        out[r:r + run] = True
        r += run + gap
        run = run % 17 + 1
        gap = gap % 9 + 1
    return out


def extra_masks(rng, n, chunk_len, D):
    """-> [(name, uint8 [nchunks, MB])]: the masks that aim at the segments' own edges, on a flat array of n elements"""
    R = chunk_len // D
    MB = -(-R // 8)
    rows = chunk_rows(n, chunk_len, D)
    nchunks = len(rows)
    masks = [("0x55", np.full((nchunks, MB), 0x55, np.uint8)), ("0xAA", np.full((nchunks, MB), 0xAA, np.uint8))]
    edge = np.zeros((nchunks, MB), np.uint8)               # rows 7 and 8 of every 16: a run of 2 rows across every second block edge ...
    edge[:, 0::2] = 0x80
    edge[:, 1::2] = 0x01
    masks.append(("0x80 0x01", edge))
    masks.append(("0x01 0x80", np.roll(edge, 1, axis=1)))  # ... and across the others
    masks.append(("ruler", pack_bits(np.stack([np.roll(ruler_bits(MB * 8), 3 * c) for c in range(nchunks)]))))
    seam = np.zeros((nchunks, MB * 8), bool)               # the last existing row and row 0 of every chunk: a segment to the chunk's end, one from its start
    for c, have in enumerate(rows):
        seam[c, 0] = True
        if have:
            seam[c, have - 1] = True
    masks.append(("last row and row 0", pack_bits(seam)))
    exist = np.zeros((nchunks, MB * 8), bool)
    for c, have in enumerate(rows):
        exist[c, :have] = True
    masks.append(("padding alone", ~pack_bits(exist)))     # every existing row clear; the padding bits and the rows that do not exist set
    masks.append(("p=1/2, padding set", pack_bits(rng.random((nchunks, MB * 8)) < 0.5) | ~pack_bits(exist)))
    return masks
