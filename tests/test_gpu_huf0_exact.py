"""GPU tests (-m gpu): the exact Huff0 writer (sprintz_mi355x_huf0_compress_batch_exact, csrc/huf0_exact.h) writes,
per chunk, the bytes of libzstd 1.4.8's HUF_compress2 -- against the committed libzstd blocks, the model
(tests/huf0_exact_model.py) and, where the library is there, the live library."""
import os
import sys

import numpy as np
import pytest

from harness import Zstd
from huf0_exact_model import huf_compress_exact

pytestmark = pytest.mark.gpu


def _run(chunks, table_log=11, align=1, pad=0):
    """host byte arrays -> (blocks, block offsets) from the GPU writer; chunk starts rounded to `align`, `pad` bytes in front"""
    import torch
    from sprintz_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    n = len(chunks)
    sizes = np.array([c.size for c in chunks], np.uint32)
    offs = np.zeros(n + 1, np.uint64)
    offs[0] = pad
    offs[1:] = pad + np.cumsum((sizes.astype(np.int64) + align - 1) // align * align)
    dense = np.zeros(int(offs[-1]) + 16, np.uint8)
    for c, o in zip(chunks, offs[:-1]):
        dense[int(o):int(o) + c.size] = c
    d_dense = torch.from_numpy(dense).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_sizes = torch.from_numpy(sizes.view(np.int32)).cuda()
    cap = int(_lib.huf0_bound(int(sizes.sum()), n))
    blocks = torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    bo = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    tmp = torch.empty(int(_lib.huf0_exact_tmp_bytes(n)), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.huf0_compress_batch_exact(d_dense.data_ptr(), d_offs.data_ptr(), d_sizes.data_ptr(), n, table_log,
                                              blocks.data_ptr(), bo.data_ptr(), tmp.data_ptr(), None))
    torch.cuda.synchronize()
    bo_h, got = bo.cpu().numpy(), blocks.cpu().numpy()
    assert (got[int(bo_h[-1]):] == 0xEE).all()                              # nothing written past the last block
    return [got[int(bo_h[c]):int(bo_h[c + 1])] for c in range(n)], blocks, bo


def _zstd_1_4_8():
    try:
        z = Zstd()
        z.z.HUF_compress2
    except (OSError, AttributeError):
        return None
    return z if z.version == 10408 else None


def test_committed_blocks_from_their_plains(golden_huf0):
    """all 372 golden plains in one batch per table log: every block equals libzstd's committed one"""
    manifest, arrays = golden_huf0
    for tl in (11, 12):
        sel = [m for m in manifest if m["name"].startswith("log12") == (tl == 12)]
        plains = [arrays["p%04d" % m["idx"]] for m in sel]
        got, _, _ = _run(plains, tl)
        for m, g in zip(sel, got):
            want = arrays["b%04d" % m["idx"]]
            assert g.size == want.size and np.array_equal(g, want), m
    assert len(manifest) == 372


def _edge_chunks(rng):
    out = []
    for n in (0, 1, 11, 12, 13, 100, 3000, 128 * 1024, 128 * 1024 + 1):
        for k in (1, 2, 20, 128, 129, 256):
            p = 1.0 / np.arange(1, k + 1) ** 1.3
            x = rng.choice(k, n, p=p / p.sum()).astype(np.uint8)
            if n >= k:
                x[:k] = np.arange(k)
            out.append(x)
    f = [1, 1]                                                             # Fibonacci counts: the length limit
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    out.append(rng.permutation(np.repeat(np.arange(22), f)).astype(np.uint8))
    out.append(rng.integers(0, 256, 5000).astype(np.uint8))              # incompressible
    out.append(np.full(9000, 7, np.uint8))
    return out


@pytest.mark.parametrize("align,pad,table_log", [(1, 0, 11), (1, 3, 11), (16, 0, 11), (1, 5, 12), (1, 0, 8)])
def test_edge_and_ragged_batches(align, pad, table_log):
    """the edge sizes, a ragged mix of stored / one-byte / 4-bit / FSE blocks, chunk starts not 16-byte aligned"""
    rng = np.random.default_rng(31 + align + pad + table_log)
    chunks = _edge_chunks(rng)
    chunks = [chunks[i] for i in rng.permutation(len(chunks))] * 2
    got, blocks, bo = _run(chunks, table_log, align, pad)
    stats = {}
    z = _zstd_1_4_8()
    for c, g in zip(chunks, got):
        want = huf_compress_exact(c, table_log, stats)
        assert g.size == want.size and np.array_equal(g, want), (c.size, g.size, want.size)
        if z is not None:
            assert np.array_equal(g, z.huf_compress(c, table_log))
    kinds = {"stored": 0, "one": 0, "coded": 0}
    for c, g in zip(chunks, got):
        if c.size:
            kinds["stored" if g.size == c.size else "one" if g.size == 1 else "coded"] += 1
    assert kinds["stored"] and kinds["one"] and stats.get("fse") and stats.get("nibbles"), (kinds, stats)
    # and back through the GPU reader
    import torch
    import sprintz_amd
    oo = np.zeros(len(chunks) + 1, np.int64)
    oo[1:] = np.cumsum([c.size for c in chunks])
    rets = torch.empty(len(chunks), dtype=torch.int64, device="cuda")
    out = sprintz_amd.huf0_decompress(blocks, bo, torch.from_numpy(oo).cuda(), rets=rets).cpu().numpy()
    assert np.array_equal(rets.cpu().numpy(), oo[1:] - oo[:-1])
    assert np.array_equal(out[: oo[-1]], np.concatenate(chunks))


def _cfg4(nchunks, seed):
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    from synth import synth_torch
    return synth_torch("walk", 2, nchunks, 5120 // 8, 8, "cuda:0", seed=seed, step=8, chunk0=0)


def test_cfg4_streams_model_libzstd_round_trip_ratio():
    """cfg4 shape (u16 x 8, FIRE, 10 KB chunks), 10 000 chunks: the blocks are the model's (a strided sample) and live
    libzstd's (all of them, where it is 1.4.8); they decode to the streams and on to the samples; the ratio is at least
    the shared-table writer's"""
    import torch
    import sprintz_amd
    nchunks = 10000
    x = _cfg4(nchunks, 123)
    cd = sprintz_amd.ChunkedCodec("xff", 2, 8, 5120, device="cuda:0")
    batch = cd.compress(x)
    blocks, bo = sprintz_amd.huf0_compress_exact(batch)
    torch.cuda.synchronize()
    comp, offs, sz_h = batch.data.cpu().numpy(), batch.offsets.cpu().numpy(), batch.sizes.cpu().numpy()
    bo_h, blk = bo.cpu().numpy(), blocks.cpu().numpy()
    streams = [comp[int(offs[c]):int(offs[c]) + int(sz_h[c])] for c in range(nchunks)]
    got = [blk[int(bo_h[c]):int(bo_h[c + 1])] for c in range(nchunks)]
    for c in range(0, nchunks, 37):
        want = huf_compress_exact(streams[c])
        assert np.array_equal(got[c], want), c
    z = _zstd_1_4_8()
    if z is not None:
        for c in range(nchunks):
            assert np.array_equal(got[c], z.huf_compress(streams[c])), c
    # round trip: blocks -> streams -> samples
    sizes = batch.sizes.to(torch.int64)
    oo = torch.zeros(nchunks + 1, dtype=torch.int64, device="cuda")
    oo[1:] = torch.cumsum(sizes, 0)
    rets = torch.empty(nchunks, dtype=torch.int64, device="cuda")
    dec = sprintz_amd.huf0_decompress(blocks, bo, oo, rets=rets)
    assert torch.equal(rets, sizes)
    out = torch.empty(nchunks * 5120, dtype=torch.uint16, device="cuda")
    cd.decompress_into(dec, oo, nchunks, out)
    assert torch.equal(out.view(torch.int16), x.view(torch.int16))
    # ratio against the shared-table writer
    _, bo_shared = sprintz_amd.huf0_compress(batch)
    exact, shared = int(bo_h[-1]), int(bo_shared[-1].item())
    print(f"cfg4 x {nchunks}: exact writer {x.numel() * 2 / exact:.4f}, shared tables {x.numel() * 2 / shared:.4f}")
    assert exact <= shared
