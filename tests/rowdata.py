"""Data, shapes and masks that the row operations' tests share: the generators and the batch builder of the windowed query's tests, the
parity tables (which ndims meets which chunk shape, data and layout), the row masks and bound sets of the filter and select tests, the
weight sets of the linear filter, the shapes named for the planner, and bench.py's inputs for the tools that time an operation."""
import numpy as np

import filter_model as fm
import linear_model as lm
from harness import DTYPES, gen_sparse


# ------------------------------------------------------------------ the windowed query's
NDIMS = [1, 2, 3, 4, 5, 8, 16, 33, 80, 128, 200, 256, 300, 512]
SHAPES = ["r16", "tail", "nogroups", "ragged"]
DATA = ["walk", "uniform", "constant", "sparse"]


def lowdim(esz, D):
    return D <= (4 if esz == 1 else 2)


def chunk_len_for(shape, D):
    r16 = 16 * max(2, 2048 // (16 * D))
    if shape == "r16":
        return D * r16
    if shape == "tail":                                   # a verbatim tail of 1 .. 15 rows
        return D * (r16 + 1 + D % 15)
    if shape == "nogroups":                               # shorter than one group of 16 rows
        return 16 * D - 3 if D > 1 else 13
    return D * r16 + max(1, D // 3)                       # chunk_len % ndims != 0 (for D = 1: one more row)


def gen_data(kind, rng, n, esz, D):
    top = 1 << (8 * esz)
    if kind == "uniform":
        return rng.integers(0, top, n).astype(DTYPES[esz])
    if kind == "constant":
        return np.full(n, 0xA5 if esz == 1 else 0x1234, DTYPES[esz])
    if kind == "sparse":
        return gen_sparse(rng, n, esz, 0.05)
    # walk of +-8 with flat spans of 150 rows (longer than a window): delta runs that cross window edges
    rows = -(-n // D)
    steps = rng.integers(-8, 9, size=(rows, D), dtype=np.int64)
    steps[(np.arange(rows) // 150) % 3 == 1] = 0
    x = np.cumsum(steps, axis=0) + rng.integers(0, top, size=(1, D))
    return np.mod(x, top).astype(DTYPES[esz]).ravel()[:n]


def make_batch(sz, oracle, codec, esz, D, chunk_len, x, general):
    """the container as ChunkedCodec.compress builds it; general layout for low-dim shapes from the oracle's
    *_rowmajor_*_rle_* writer (the batched encoders write sprintz.h's layout, which is the general one from 5 / 3 columns on)"""
    import torch
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device="cuda:0")
    if not (general and lowdim(esz, D)):
        return cd, cd.compress(torch.from_numpy(x.view(np.int8 if esz == 1 else np.int16)).cuda().view(cd.dtype))
    n = x.size
    nchunks = -(-n // chunk_len)
    streams = [oracle.compress_rowmajor(codec, x[c * chunk_len:(c + 1) * chunk_len], D)[0] for c in range(nchunks)]
    offs = np.zeros(nchunks + 1, np.int64)
    for c, s in enumerate(streams):
        offs[c + 1] = (offs[c] + s.size + 15) & ~15
    data = np.zeros(int(offs[-1]) + sz._lib.READ_SLACK, np.uint8)
    for c, s in enumerate(streams):
        data[offs[c]:offs[c] + s.size] = s
    batch = sz.CompressedBatch(torch.from_numpy(data).cuda(), torch.from_numpy(offs).cuda(),
                               torch.tensor([s.size for s in streams], dtype=torch.int32).cuda(), nchunks, n, chunk_len, D)
    return cd, batch


def parity_cases():
    """codec x esz x ndims in full; per (codec, esz) the 14 ndims walk the chunk shapes, data and layouts so that every
    value of every axis meets both codecs and both widths; each case is queried at all five windows on both families"""
    cases = []
    for codec in ("delta", "xff"):
        for esz in (1, 2):
            for j, D in enumerate(NDIMS):
                shape = SHAPES[j % 4]
                data = DATA[(j + (1 if codec == "xff" else 0) + 2 * (esz - 1)) % 4]
                general = (j // 2 + esz) % 2 == 1
                cases.append((codec, esz, D, shape, data, general))
    return cases


# ------------------------------------------------------------------ the filter's

def existing_rows(x, chunk_len, D):
    """[rows, D]: the rows that exist, chunk by chunk (columns are relative to the chunk: element e of a chunk is column e % D)"""
    parts = []
    for c, ne in enumerate(fm.chunk_counts(x.size, chunk_len)):
        parts.append(x[c * chunk_len:c * chunk_len + ne // D * D].reshape(-1, D))
    return np.concatenate(parts)


def bound_sets(x, chunk_len, esz, D):
    """-> [(name, mode, lo, hi, expectation)]; expectation: "some" (strictly between no row and every row), "all", "none" or None"""
    top = (1 << (8 * esz)) - 1
    rows = existing_rows(x, chunk_len, D).astype(np.int64)
    sets = []
    lo, hi = np.zeros(D, np.int64), np.full(D, top, np.int64)              # band: columns 0 and D - 1 inside their own quartiles
    for d in (0, D - 1):
        lo[d], hi[d] = np.quantile(rows[:, d], 0.25, method="lower"), np.quantile(rows[:, d], 0.75, method="lower")
    sets.append(("band", fm.ALL, lo, hi, "some"))
    t = int(np.quantile(x.astype(np.int64), 1.0 - 1.0 / (4 * D), method="higher"))   # alarm: some channel in the top 1 / (4 D) of the input
    sets.append(("alarm", fm.ANY, np.full(D, t, np.int64), np.full(D, top, np.int64), "some"))
    sets.append(("all rows", fm.ALL, np.zeros(D, np.int64), np.full(D, top, np.int64), "all"))
    sets.append(("no row", fm.ANY, np.full(D, top, np.int64), np.zeros(D, np.int64), "none"))
    lo, hi = np.zeros(D, np.int64), np.full(D, top, np.int64)              # one column never, under ALL: no row
    lo[D // 2], hi[D // 2] = 1, 0
    sets.append(("one never", fm.ALL, lo, hi, "none"))
    lo, hi = np.full(D, top, np.int64), np.zeros(D, np.int64)              # one column always, under ANY: every existing row
    lo[D // 2], hi[D // 2] = 0, top
    sets.append(("one always", fm.ANY, lo, hi, "all"))
    return sets, rows.shape[0]


# ------------------------------------------------------------------ select rows'

def short_batch(nchunks, chunk_len, D):
    """elements of a batch of nchunks chunks whose last one is short by a third of its rows (whole rows)"""
    R = chunk_len // D
    return nchunks * chunk_len - max(1, R // 3) * D


def parity_masks(rng, x, chunk_len, esz, D):
    """-> [(name, mask)] of the module docstring's list"""
    R, MB = fm.geometry(chunk_len, D)
    lens = fm.chunk_counts(x.size, chunk_len)
    nchunks = len(lens)
    sets, _ = bound_sets(x, chunk_len, esz, D)
    masks = []
    for name, mode, lo, hi, _ in sets[:3]:                 # band, alarm, all rows
        masks.append((name, fm.filter_rows(x, chunk_len, D, lo, hi, mode)[0]))
    masks.append(("no row", np.zeros((nchunks, MB), np.uint8)))
    for name, p in (("p=1/2", 0.5), ("p=1/64", 1.0 / 64)):
        masks.append((name, np.packbits(rng.random((nchunks, MB * 8)) < p, axis=1, bitorder="little")))

    def from_rows(pick):
        bits = np.zeros((nchunks, MB * 8), np.uint8)
        for c, ne in enumerate(lens):
            bits[c, pick(ne // D)] = 1
        return np.packbits(bits, axis=1, bitorder="little")
    masks.append(("row 0", from_rows(lambda have: [0])))
    masks.append(("last row", from_rows(lambda have: [have - 1])))
    masks.append(("tail rows", from_rows(lambda have: np.arange(have // 16 * 16 if have % 16 else have - min(have, 16), have))))
    alt = np.zeros((nchunks, MB), np.uint8)
    alt[:, 1::2] = 0xFF
    masks.append(("alternating bytes", alt))
    masks.append(("every bit", np.full((nchunks, MB), 0xFF, np.uint8)))
    return masks


# ------------------------------------------------------------------ aggregate rows' (and the other masked operations')

MASKED_NDIMS = [1, 2, 3, 4, 5, 8, 16, 33, 80, 128, 256, 300, 512]
MASKED_SHAPES = ["r16", "tail", "nogroups"]


# the parity shapes decode_fast.h takes, as (esz, D, general layout asked for); the planner's edges are pinned in each operation's CPU tests
PARITY_FAST = {(1, 4, True), (1, 16, False), (2, 4, False), (2, 16, False)}


def rows_for(shape, D):
    r16 = 16 * max(2, 2048 // (16 * D))
    return {"r16": r16, "tail": r16 + 1 + D % 15, "nogroups": 13}[shape]     # whole groups; a verbatim tail of 1 .. 15 rows; no groups


def windows_for(R):
    r8 = -(-R // 8) * 8
    return sorted({8, 24, 64, r8, r8 + 8})


def masked_parity_cases():
    """codec x esz x ndims in full; per (codec, esz) the ndims walk the three chunk shapes and the four kinds of data"""
    cases = []
    for codec in ("delta", "xff"):
        for esz in (1, 2):
            for j, D in enumerate(MASKED_NDIMS):
                cases.append((codec, esz, D, MASKED_SHAPES[j % 3], DATA[(j + (1 if codec == "xff" else 0) + 2 * (esz - 1)) % 4]))
    return cases


FAST_SHAPES = [
    # (codec, esz, D, chunk_len): decode_fast.h's lane mappings -- 4 .. 64 lanes a chunk, 1 / 2 / 4 columns a lane, full and partly filled groups
    ("xff", 2, 8, 5120), ("delta", 2, 8, 8 * 648), ("delta", 2, 5, 5 * 1000), ("xff", 1, 8, 8 * 1024), ("delta", 1, 24, 24 * 200),
    ("xff", 2, 24, 24 * 200), ("xff", 1, 64, 64 * 160), ("delta", 1, 80, 10240), ("xff", 2, 80, 80 * 128), ("delta", 2, 128, 128 * 80),
    ("xff", 1, 200, 200 * 104), ("delta", 1, 256, 256 * 80),
]


# ------------------------------------------------------------------ histogram and group-by rows'

HS = (0, 1, 2, 3)               # one histogram; one a chunk; two chunks; three: cuts every workgroup's chunk range in the middle


# ------------------------------------------------------------------ the linear filter's

def quartiles(s):
    return int(np.quantile(s, 0.25, method="lower")), int(np.quantile(s, 0.75, method="lower"))


def weight_sets(rng, x, esz, D, lag):
    """-> [(name, w, u, bias, lo, hi)]: the issue's six, with (lag) or without a lag term.  Bounds are quantiles of the model's sums, so
    that a predicate splits the rows; they are inputs, not tolerances."""
    top = (1 << (8 * esz)) - 1
    e = np.eye(D, dtype=np.int64)
    sets = []
    w = e[D - 1]
    u = -w if lag else None
    sets.append(("single", w, u, 0) + quartiles(lm.sums(x, D, w, u)))
    w = e[0] - e[D - 1] if D > 1 else e[0]
    u = -w if lag else None
    sets.append(("a - b", w, u, 0, 1, None))                                   # a > b (lag: a - b grew)
    w = np.ones(D, np.int64)
    u = -w if lag else None
    sets.append(("ones", w, u, 0) + quartiles(lm.sums(x, D, w, u)))
    terms = D * (2 if lag else 1)
    wmax = ((1 << 31) - 1) // (top * terms)
    w = rng.integers(-wmax, wmax + 1, D)
    u = rng.integers(-wmax, wmax + 1, D) if lag else None
    bias = (1 << 31) - 1 - lm.bound_B(esz, w, u)                               # what is left of the bound goes into the bias: B = 2^31 - 1
    bias = -bias if rng.integers(2) else bias
    assert lm.bound_B(esz, w, u, bias) == (1 << 31) - 1, ("the random weights' bound B is not 2^31 - 1", lm.bound_B(esz, w, u, bias))
    sets.append(("random", w, u, bias) + quartiles(lm.sums(x, D, w, u, bias)))
    w = e[D // 2]
    u = -w if lag else None
    v = int(np.quantile(lm.sums(x, D, w, u), 0.5, method="lower"))
    sets.append(("equal", w, u, 0, v, v))
    sets.append(("nothing", np.ones(D, np.int64), u, 3, 5, 4))
    return sets


# ------------------------------------------------------------------ bench.py's inputs

def bench_input(name, device):
    """exactly what bench.py's run_config(name) / headline generates on rank 0 of 1"""
    import torch
    from synth import synth_torch
    if name == "cfg2":
        return ("xff", 2, 8, 5120, 131072), synth_torch("walk", 2, 131072, 640, 8, device, seed=123, step=8, chunk0=0)
    if name.startswith("cfg2_"):               # bench.py's data_sweep: the headline shape on SURVEY 8d's other generators
        kind, step = {"cfg2_uniform": ("uniform", 0), "cfg2_walk300": ("walk", 300), "cfg2_walkflat": ("walkflat", 8)}[name]
        return ("xff", 2, 8, 5120, 131072), synth_torch(kind, 2, 131072, 640, 8, device, seed=123, step=step, chunk0=0)
    if name == "cfg1":
        return ("delta", 1, 1, 1024, 524288), synth_torch("walk", 1, 524288, 1024, 1, device, seed=123, step=2, chunk0=0)
    if name == "cfg3_10k":
        return ("delta", 1, 80, 10240, 52429), synth_torch("walk", 1, 52429, 128, 80, device, seed=123, step=2, chunk0=0)
    if name == "cfg3_1k":                      # 1024 elements do not hold whole rows of 80: 64-row series, cut every 1024
        from synth import synth_cut_rows
        return ("delta", 1, 80, 1024, 524288), synth_cut_rows("walk", 1, 524288, 1024, 80, device, seed=123, step=2)
    raise ValueError(name)


# ------------------------------------------------------------------ the ragged shapes of the CPU model tests

RAGGED_SHAPES = [
    # (esz, D, chunk_len, n): whole rows, short last chunks (one ending mid-row), R % 8 != 0 and R < 8
    (1, 3, 3 * 33, 3 * 33 * 4 + 3 * 14),
    (2, 5, 5 * 21, 5 * 21 * 3 + 5 * 4 + 2),
    (1, 1, 13, 13 * 5 + 6),
    (2, 8, 8 * 64, 8 * 64 * 3),
    (1, 7, 7 * 5, 7 * 5 * 6 + 7),
]


# ------------------------------------------------------------------ float rows'

# the shapes the issue names: rows of whole 16-byte pieces, and rows that are not (the low-dim layouts among them)
FLOAT_FAST_SHAPES = [(2, 8), (2, 16), (2, 24), (2, 64), (2, 128), (1, 16), (1, 80), (1, 256)]
GENERIC_SHAPES = [(2, 1), (2, 2), (2, 3), (2, 5), (2, 12), (1, 1), (1, 4), (1, 7)]
