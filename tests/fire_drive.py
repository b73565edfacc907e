"""Inputs that STEER the FIRE forecaster's counters -- through the int16 wrap of the 8-bit counter and past 2^23
with the 16-bit low-dim coefficient -- where every other input of the suite lets them drift like a random walk of a few dozen a block.

Plain numpy; nothing here is product code or oracle code.  A sequential generator, vectorised over columns, carries the forecaster's
state (prev_val, prev_delta, counter) per column -- the arithmetic of kat.fire_coefficients -- and picks each row's delta from the forecast:

  even rows of a block   delta = +B in an "up" column, -(B + 1) in a "down" one, B = 2^(w-3) - 1 (31 / 8 191): four such terms fit the
                         w-bit gradient without wrapping
  odd rows               delta = wrap_w(pred + e), e drawn from 1 .. 3: the error is positive, the gradient term is prev_delta, and the
                         counter moves +31 / -32 (+8 191 / -8 192) every block
  run spans              delta = pred in every column and row: zero errors, RUN blocks, and the decoder must replay the forecast with whatever
                         coefficient is frozen at that point (counters only move on real blocks)

The counters returned (the one each block STARTED with) are for coverage assertions only; expected bytes are always the oracle's.

transform=True is the stand-alone transform's forecaster at 8 bits (csrc/transforms.hip xff_kernel, oracle/transforms_oracle.c): the
general layout's coefficient, and pred = byte 1 of the 16-bit product m * coef with m the previous delta taken SIGNED in odd columns and
UNSIGNED in even ones."""
from functools import lru_cache

import numpy as np

from kat import _wrap

NB8 = 1160                     # 8 bits: an up column wraps after 1 058 driven blocks, a down column after 1 025; 50 run blocks
NB16 = 4400                    # 16-bit low-dim: counters of +-36 M, coefficients of +-18 M (2^23 is 8.4 M)
# (first block, one past the last) of the run spans.  8 bits: |coef| >= 8 192 from about block 530 on; the down columns wrap at block 1 047,
# the up columns at 1 088: one span before every wrap, one within 10 blocks of the first, one behind the last
RUNS8 = ((600, 622), (1052, 1060), (1100, 1120))
RUNS16 = ((2100, 2120), (4300, 4330))          # both behind |coef| = 2^23 (block 2 049)
TILE = 64                      # wide inputs: this many distinct column trajectories, tiled (columns are independent, the spans common)


def coefficient(counter, w, lowdim):
    """sprintz_xff_lowdim.cpp:170-173 (untruncated) / sprintz_xff_rle.cpp:217 (the top bits, as an int16)"""
    counter = np.asarray(counter, np.int64)
    if lowdim:
        return counter >> 1
    return _wrap((counter >> (1 + (w - 4))) << (w - 4), 16)


def _predict(prev_delta, coef, w, transform, odd_col):
    if transform:
        m = np.where(odd_col, prev_delta, prev_delta & 0xff)
        return _wrap(((m * coef) >> 8) & 0xff, 8)
    return _wrap(_wrap(prev_delta * coef, 32) >> w, w)


def _drive(w, lowdim, dirs, seed, nblocks, runs, transform):
    assert w in (8, 16) and not (transform and (w != 8 or lowdim))
    dirs = np.asarray(dirs, np.int64)
    nd = dirs.size
    rng = np.random.default_rng(seed)
    B = (1 << (w - 3)) - 1
    cbits = 16 if w == 8 else 32
    push = np.where(dirs > 0, B, -(B + 1))
    odd_col = (np.arange(nd) & 1) == 1
    if isinstance(runs, np.ndarray):                 # per column: [nblocks, ncols] bool (tests/rle_drive.py lays chunks out side by side)
        in_run = runs.reshape(nblocks, -1)
    else:
        in_run = np.zeros((nblocks, 1), bool)
        for a, b in runs:
            in_run[a:b] = True
    e_all = rng.integers(1, 4, size=(nblocks, 4, nd))
    prev_val = np.zeros(nd, np.int64)
    prev_delta = np.zeros(nd, np.int64)
    counter = np.zeros(nd, np.int64)
    x = np.empty((8 * nblocks, nd), np.int64)
    counters = np.empty((nblocks, nd), np.int64)
    errs = np.empty((8 * nblocks, nd), np.int64)
    for b in range(nblocks):
        counters[b] = counter
        coef = coefficient(counter, w, lowdim)
        grad = np.zeros(nd, np.int64)
        for i in range(8):
            pred = _predict(prev_delta, coef, w, transform, odd_col)
            if i & 1:
                delta = np.where(in_run[b], pred, _wrap(pred + e_all[b, i >> 1], w))
            else:
                delta = np.where(in_run[b], pred, push)
            err = _wrap(delta - pred, w)
            if i & 1:
                grad = _wrap(grad + _wrap(np.sign(err) * prev_delta, w), w)
            prev_val = (prev_val + delta) & ((1 << w) - 1)
            prev_delta = delta
            x[8 * b + i] = prev_val
            errs[8 * b + i] = err
        counter = _wrap(counter + (grad >> 2), cbits)
    dt = np.uint8 if w == 8 else np.uint16
    return x.astype(dt), counters, (errs & ((1 << w) - 1)).astype(dt)


@lru_cache(maxsize=None)
def _cached(w, lowdim, dirs, seed, nblocks, runs, transform):
    out = _drive(w, lowdim, dirs, seed, nblocks, runs, transform)
    for a in out:
        a.setflags(write=False)
    return out


def drive(w, lowdim, dirs, seed, nblocks, runs=(), transform=False):
    """dirs: per column +1 (up) / -1 (down) -> (samples [8 * nblocks, ncols], counters [nblocks, ncols], the model's errors like the samples);
    read-only arrays, cached per process.  runs may also be a bool array [nblocks, ncols] -- a schedule of each column's own (not cached)"""
    if isinstance(runs, np.ndarray):
        return _drive(int(w), bool(lowdim), dirs, int(seed), int(nblocks), np.asarray(runs, bool), bool(transform))
    return _cached(int(w), bool(lowdim), tuple(int(d) for d in dirs), int(seed), int(nblocks), tuple((int(a), int(b)) for a, b in runs), bool(transform))


def directions(ncols, pattern):
    """pattern 0: all up; 1: all down; 2: alternating from up; 3: alternating from down; 4 and up: a fixed pseudo-random mix that starts up, down"""
    c = np.arange(ncols)
    if pattern == 0:
        return tuple([1] * ncols)
    if pattern == 1:
        return tuple([-1] * ncols)
    if pattern in (2, 3):
        return tuple(int(v) for v in np.where((c + pattern) & 1, -1, 1))
    d = np.where(np.random.default_rng(7000 + pattern).random(ncols) < 0.5, 1, -1)
    d[:2] = (1, -1)[:ncols]
    return tuple(int(v) for v in d)


def is_lowdim(w, ncols):
    return ncols <= (4 if w == 8 else 2)


def chunk(w, ncols, seed, pattern, runs=None, nblocks=None, transform=False):
    """one chunk of the codec's (or the transform's) layout for that width and column count, with the module's run spans unless given
    -> (samples [rows, ncols], counters [nblocks, ncols]).  Columns are independent and the run spans common to all, so every column count
    of a layout shares one generated set of trajectories per (seed, pattern): the first ncols of the low-dim layout's 4 (2 at 16 bits) or of
    the general layout's TILE, tiled beyond that (TILE is even: a column keeps the parity the transform's forecast depends on)"""
    lowdim = is_lowdim(w, ncols) and not transform
    runs = (RUNS8 if w == 8 else RUNS16) if runs is None else runs
    nblocks = (NB8 if w == 8 else NB16) if nblocks is None else nblocks
    gen = (4 if w == 8 else 2) if lowdim else TILE
    x, ctr, _ = drive(w, lowdim, directions(gen, pattern), seed, nblocks, runs, transform)
    if ncols > gen:
        reps = -(-ncols // gen)
        x, ctr = np.tile(x, (1, reps)), np.tile(ctr, (1, reps))
    return x[:, :ncols], ctr[:, :ncols]


def batch(w, ncols, nchunks, seed0=0, runs=None, nblocks=None):
    """nchunks chunks with seeds and direction patterns of their own (the lanes of a wave sit at different counter states); chunk 0 is
    chunk(w, ncols, seed0, 2), the golden fixture's case -> flat samples"""
    parts = [chunk(w, ncols, seed0 + k, (2, 3, 0, 1, 4, 5, 6)[k % 7], runs, nblocks)[0] for k in range(nchunks)]
    return np.concatenate([p.ravel() for p in parts])


def wraps(counters):
    """[nblocks - 1, ncols] bool: the counter jumped by more than 30 000 between two blocks (an int16 wrap: a block moves it by 32 at most)"""
    return np.abs(np.diff(np.asarray(counters, np.int64), axis=0)) > 30000


# the cases of tests/golden/golden_firewrap_v1 (oracle/gen_golden_firewrap.py): chunk(w, ncols, GOLDEN_SEED, GOLDEN_PATTERN)
GOLDEN_SEED, GOLDEN_PATTERN = 0, 2
GOLDEN_CODEC = ((8, 1), (8, 3), (8, 8), (16, 2))          # (w, ncols) of the codec's streams
GOLDEN_TRANSFORM = ((8, 1), (8, 8))                      # ... of the stand-alone transform's containers


def codec_input(w, ncols, seed=GOLDEN_SEED, pattern=GOLDEN_PATTERN):
    """flat samples of one chunk, for the codec"""
    return np.ascontiguousarray(chunk(w, ncols, seed, pattern)[0]).ravel()


def transform_input(ncols, seed=GOLDEN_SEED, pattern=GOLDEN_PATTERN):
    """9 280 rows steered against the transform's forecaster and 5 samples of a ragged last row: the transform leaves its last blocks to
    plain delta coding whenever its vector stores would spill (predict.cpp:96-103), so the tail differs from the model by design"""
    x = chunk(8, ncols, seed, pattern, transform=True)[0]
    return np.concatenate([x.ravel(), (np.arange(5) * 37 + 11).astype(np.uint8)])


def transform_forecast_blocks(n, ncols):
    """predict.cpp:96-103 at 8 bits, as oracle/transforms_oracle.c states it"""
    nblocks = (n // ncols) // 8
    overrun = 32 - ncols % 32
    if overrun > n % (8 * ncols):
        nblocks = max(0, nblocks - -(-overrun // (8 * ncols)))
    return nblocks
