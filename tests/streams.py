"""Option sets and stream checks of the row-major kernel families: the knobs that choose a family (options, OLD / DEF / DENSE / GENERIC), the
FIRE drive's batches as the oracle's containers, the comparison of a container's streams with the oracle's, and a container with one
truncated stream (truncated_batch)."""
import os
from contextlib import contextmanager
from functools import lru_cache

import numpy as np

import fire_drive as fd


# ------------------------------------------------------------------ stream checks


def check_streams(oracle, codec, data, chunk_len, D, comp, offs, sizes, tag):
    want = oracle.compress_chunks(codec, data, chunk_len, D)
    assert len(want) == sizes.size, (tag, "chunks", sizes.size, "the oracle's", len(want))
    for c, w in enumerate(want):
        assert sizes[c] == w.size, (tag, c, int(sizes[c]), w.size)
        assert np.array_equal(comp[offs[c]:offs[c] + sizes[c]], w), (tag, "chunk", c, "differs from the oracle's stream")


def truncated_batch(sz, batch, cut):
    """the container with chunk `cut`'s stream 5 bytes short, the streams packed densely again"""
    import torch
    n = batch.nchunks
    comp, offs, sizes = batch.data.cpu().numpy(), batch.offsets.cpu().numpy(), batch.sizes.cpu().numpy()
    parts = [comp[offs[c]:offs[c] + sizes[c] - (5 if c == cut else 0)].copy() for c in range(n)]
    toffs = np.zeros(n + 1, np.int64)
    toffs[1:] = np.cumsum([p.size for p in parts])
    return sz.CompressedBatch(torch.from_numpy(np.concatenate(parts + [np.zeros(sz._lib.READ_SLACK, np.uint8)])).cuda(), torch.from_numpy(toffs).cuda(),
                              torch.tensor([p.size for p in parts], dtype=torch.int32).cuda(), n, batch.total_len, batch.chunk_len, batch.ndims)


# ------------------------------------------------------------------ option sets and the FIRE drive's batches


DENSE = ("dense_fused", "dense_compact", "dense_verbatim")          # how the container was built is not these cases' subject


@contextmanager
def options(lat=2048, blk_chunks=2049, mask=9, pair=1, no_fast=0, split=1):
    """the knobs the row-major dispatch reads, at the library's defaults unless given (pair: the test session's, tests/conftest.py)"""
    from sprintz_amd import _lib
    knobs = [(_lib.OPT_LAT_CHUNKS, lat, "SPRINTZ_MI355X_LAT_CHUNKS", 2048), (_lib.OPT_BLK_CHUNKS, blk_chunks, "SPRINTZ_MI355X_BLK_CHUNKS", 2049),
             (_lib.OPT_BLK_KERNELS, mask, "SPRINTZ_MI355X_BLK_KERNELS", 9), (_lib.OPT_ENC_PAIR, pair, "SPRINTZ_MI355X_ENC_PAIR", 1024),
             (_lib.OPT_SPLIT_LANES, split, "SPRINTZ_MI355X_SPLIT_LANES", 1)]
    for opt, v, _, _ in knobs:
        _lib.check(_lib.set_option(opt, v))
    _lib.check(_lib.set_option(_lib.OPT_NO_FAST, no_fast))
    try:
        yield
    finally:
        for opt, _, env, default in knobs:
            _lib.set_option(opt, int(os.environ.get(env, default)))
        _lib.set_option(_lib.OPT_NO_FAST, 1 if os.environ.get("SPRINTZ_MI355X_NO_FAST") is not None else 0)


@lru_cache(maxsize=None)
def fire_batch_of(w, D, nchunks, nblocks=None, runs=None):
    """(flat samples, chunk_len); read-only, shared by the cases of the module"""
    x = fd.batch(w, D, nchunks, runs=runs, nblocks=nblocks)
    x.setflags(write=False)
    return x, x.size // nchunks


def to_device(cd, data):
    import torch
    return torch.from_numpy(data.view(np.int8 if data.dtype.itemsize == 1 else np.int16).copy()).cuda().view(cd.dtype)      # (a copy: the shared arrays are read-only)


def fire_oracle_batch(sz, oracle, D, data, chunk_len):
    """the ORACLE's streams as a container (16-byte aligned, as ChunkedCodec.compress builds it): what a decoder-only case reads, so that an
    encoder and a decoder that are wrong in the same way cannot agree with each other"""
    import torch
    streams = oracle.compress_chunks("xff", data, chunk_len, D)
    offs = np.zeros(len(streams) + 1, np.int64)
    for c, s in enumerate(streams):
        offs[c + 1] = (offs[c] + s.size + 15) & ~15
    comp = np.zeros(int(offs[-1]) + sz._lib.READ_SLACK, np.uint8)
    for c, s in enumerate(streams):
        comp[offs[c]:offs[c] + s.size] = s
    return sz.CompressedBatch(torch.from_numpy(comp).cuda(), torch.from_numpy(offs).cuda(), torch.tensor([s.size for s in streams], dtype=torch.int32).cuda(),
                              len(streams), data.size, chunk_len, D)


OLD = dict(lat=0, blk_chunks=0)                        # the lane-per-column kernels alone
DEF = dict()                                           # the library's defaults: the workgroup-per-chunk kernels up to 2 048 chunks
GENERIC = dict(no_fast=1)                              # SPRINTZ_OPT_NO_FAST: encode_kernel.h / decode_kernel.h for everything up to 512 columns
