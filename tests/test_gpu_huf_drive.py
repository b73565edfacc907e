"""GPU tests (-m gpu): the shared Huffman table builder (huf_build_kernel, K1 of sprintz_amd/csrc/huf.hip) and the two writers and the
reader behind it, on tests/huf_drive.py's batches: segments of 0, 1, 2 and 3 symbols, depths 11 / 12 / 23, the 4-leaves-per-lane
boundaries at 64 / 128 / 192 leaves, 40 .. 75 lengthening and 13 shortening rounds in every quarter of the sorted leaves, repair ties that
only the symbol decides, leaf / internal ties in the merge; records on both sides of the stored rule and of the 16-bit size fields, a
fourth sub-stream above 64 KB, chunk sizes 0 .. 17 and around a workgroup's trip, sources at odd addresses, 1 / 63 / 64 / 65 / 129
chunks, containers that end on every kind of 64-byte boundary.  tests/test_huf_drive_cpu.py proves that the batches get there.

The C entry points are called directly, on sentinel-filled buffers with guard space: every byte of every output buffer is compared with
what the oracle writes into a buffer filled the same way, so bytes the kernels must NOT write (the gaps between records and chunks, the
guard) count like the ones they must.  Everything is exact."""
import numpy as np
import pytest

import huf_drive as hd
from harness import Zstd
from codec_helpers import check_case, decode_sample
from fixtures import gpu_lib as lib  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SENT, POISON, GUARD = 0xEE, 0xCD, 4096
BATCHES = list(hd.batches())
_cache = {}


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def filled(nbytes, value):
    import torch
    return torch.full((int(nbytes),), value, dtype=torch.uint8, device="cuda")


def source(bname):
    """-> (chunks, dense, offsets, sizes) of a drive batch, and the same on the device"""
    if ("src", bname) not in _cache:
        b = hd.batches()[bname]
        dense, offs, sizes = hd.layout(b["chunks"], b["align"], b["shift"])
        _cache["src", bname] = (b, dense, offs, sizes, dev(dense), dev(offs), dev(sizes))
    return _cache["src", bname]


def oracle_written(oracle, bname):
    """the oracle's container written into a sentinel-filled buffer of the GPU's size -> (buffer, huf_offsets, tables)"""
    if ("want", bname) not in _cache:
        b, dense, offs, sizes, *_ = source(bname)
        n = len(sizes)
        oracle._huf_bind()
        out = np.full(int(sizes.astype(np.int64).sum()) + 8 * n + 16 + GUARD, SENT, np.uint8)
        ho = np.zeros(n + 1, np.uint64)
        tables = np.full(((n + 63) // 64) * 128 + GUARD, SENT, np.uint8)
        oracle._huf_c(dense.ctypes.data, offs.ctypes.data, sizes.ctypes.data, n, out.ctypes.data, ho.ctypes.data, tables.ctypes.data)
        _cache["want", bname] = (out, ho, tables)
    return _cache["want", bname]


def gpu_written(lib, bname):
    """huf_compress_batch of a drive batch into sentinel-filled buffers -> (whole container buffer, huf_offsets, whole tables buffer)"""
    if ("got", bname) not in _cache:
        import torch
        b, dense, offs, sizes, d_dense, d_offs, d_sizes = source(bname)
        n = len(sizes)
        total = int(sizes.astype(np.int64).sum())
        bound = int(lib.huf_bound(total, n))
        assert bound == total + 8 * n + 16
        d_huf = filled(bound + GUARD, SENT)
        d_ho = filled(8 * (n + 1) + GUARD, SENT)
        d_tables = filled(((n + 63) // 64) * 128 + GUARD, SENT)
        d_tmp = filled(int(lib.huf_tmp_bytes(n)) + GUARD, SENT)
        lib.check(lib.huf_compress_batch(d_dense.data_ptr(), d_offs.data_ptr(), d_sizes.data_ptr(), n, d_huf.data_ptr(), d_ho.data_ptr(),
                                         d_tables.data_ptr(), d_tmp.data_ptr(), None))
        torch.cuda.synchronize()
        ho_raw = d_ho.cpu().numpy()
        assert (ho_raw[8 * (n + 1):] == SENT).all(), "huf_offsets: written behind its n + 1 entries"
        assert (d_tmp.cpu().numpy()[int(lib.huf_tmp_bytes(n)):] == SENT).all(), "scratch: written behind huf_tmp_bytes"
        _cache["got", bname] = (d_huf.cpu().numpy(), ho_raw[:8 * (n + 1)].view(np.uint64).copy(), d_tables.cpu().numpy())
    return _cache["got", bname]


def first_difference(got, want):
    d = np.flatnonzero(got != want)
    return None if d.size == 0 else (int(d[0]), int(got[d[0]]), int(want[d[0]]), int(d.size))


# ----------------------------------------------------------------- our container: the writer

@pytest.mark.parametrize("bname", BATCHES)
def test_writer_tables_offsets_and_every_byte(lib, oracle, bname):
    b, dense, offs, sizes, *_ = source(bname)
    want, want_ho, want_tables = oracle_written(oracle, bname)
    got, got_ho, got_tables = gpu_written(lib, bname)
    for sname, first in b["segments"]:                          # K1's table of every segment, named
        s = first // hd.SEG
        assert np.array_equal(got_tables[128 * s:128 * s + 128], want_tables[128 * s:128 * s + 128]), (bname, "table of segment", sname)
    assert np.array_equal(got_tables, want_tables), (bname, "tables buffer (guard included)", first_difference(got_tables, want_tables))
    assert np.array_equal(got_ho, want_ho), (bname, "huf_offsets", first_difference(got_ho, want_ho))
    # records, the gaps between them (nobody writes them) and the guard: (offset, got, want, bytes that differ)
    assert np.array_equal(got, want), (bname, "container buffer", first_difference(got, want))
    if "residue" in b:
        assert int(got_ho[-1]) % 64 == b["residue"]
    # the second opinion, on the GPU's bytes
    for case in b["cases"]:
        check_case(case, b["chunks"][case["chunk"]], got, got_ho, got_tables, who="gpu")
    decode_sample(b, got, got_ho, got_tables, who="gpu")


# ----------------------------------------------------------------- our container: the reader

def expected_dense(chunks, align, capacity=None):
    """-> (offsets, poisoned buffer with the chunks in it, rets): chunk starts rounded up to `align`, the end too; a chunk that does not
    fit `capacity` is refused and leaves the poison"""
    n = len(chunks)
    offs = np.zeros(n + 1, np.uint64)
    pos = 0
    for c, ch in enumerate(chunks):
        pos = (pos + align - 1) & ~(align - 1)
        offs[c] = pos
        pos += len(ch)
    offs[n] = (pos + align - 1) & ~(align - 1)
    cap = int(offs[n]) if capacity is None else capacity
    buf = np.full(int(offs[n]) + GUARD, POISON, np.uint8)
    rets = np.zeros(n, np.int64)
    for c, ch in enumerate(chunks):
        if int(offs[c]) + len(ch) <= cap:
            buf[int(offs[c]):int(offs[c]) + len(ch)] = ch
            rets[c] = len(ch)
        else:
            rets[c] = -5
    return offs, buf, rets


def run_reader(lib, container, ho, tables, nchunks, total_in, align, capacity, dense_bytes):
    """huf_decompress_batch of `container` held in a buffer of exactly huf_bound bytes -> (dense buffer, offsets, sizes, rets)"""
    import torch
    bound = int(lib.huf_bound(total_in, nchunks))
    assert int(ho[-1]) <= bound
    held = np.full(bound, SENT, np.uint8)
    held[:int(ho[-1])] = container[:int(ho[-1])]
    d_huf, d_ho, d_tables = dev(held), dev(ho), dev(tables[:((nchunks + 63) // 64) * 128])
    d_dense = filled(dense_bytes, POISON)
    d_offs = filled(8 * (nchunks + 1) + 64, SENT)
    d_sizes = filled(4 * nchunks + 64, SENT)
    d_rets = torch.full((nchunks + 8,), -99, dtype=torch.int64, device="cuda")
    d_tmp = filled(int(lib.huf_tmp_bytes(nchunks)), SENT)
    lib.check(lib.huf_decompress_batch(d_huf.data_ptr(), d_ho.data_ptr(), d_tables.data_ptr(), nchunks, align, d_dense.data_ptr(), capacity,
                                       d_offs.data_ptr(), d_sizes.data_ptr(), d_rets.data_ptr(), d_tmp.data_ptr(), None))
    torch.cuda.synchronize()
    o, s, r = d_offs.cpu().numpy(), d_sizes.cpu().numpy(), d_rets.cpu().numpy()
    assert (o[8 * (nchunks + 1):] == SENT).all() and (s[4 * nchunks:] == SENT).all() and (r[nchunks:] == -99).all()
    return d_dense.cpu().numpy(), o[:8 * (nchunks + 1)].view(np.uint64), s[:4 * nchunks].view(np.uint32), r[:nchunks]


@pytest.mark.parametrize("whose", ["the GPU's container", "the oracle's container"])
@pytest.mark.parametrize("bname", BATCHES)
def test_reader_at_every_alignment(lib, oracle, bname, whose):
    """offsets, sizes and rets exact, every chunk back, the poison everywhere else: between the chunks, behind the end.  dense_capacity
    is exactly offsets[n], and the container sits in a buffer of exactly huf_bound bytes (the reader's 16-byte piece loads are clamped to
    the last one that holds container bytes)."""
    b, dense, offs, sizes, *_ = source(bname)
    container, ho, tables = gpu_written(lib, bname) if whose.startswith("the GPU") else oracle_written(oracle, bname)
    n, total_in = len(sizes), int(sizes.astype(np.int64).sum())
    for align in (1, 2, 4, 8, 16):
        want_offs, want, want_rets = expected_dense(b["chunks"], align)
        got, got_offs, got_sizes, got_rets = run_reader(lib, container, ho, tables, n, total_in, align, int(want_offs[-1]), want.size)
        assert np.array_equal(got_offs, want_offs), (bname, align, "offsets", first_difference(got_offs, want_offs))
        assert np.array_equal(got_sizes, sizes), (bname, align, "sizes", first_difference(got_sizes, sizes))
        assert np.array_equal(got_rets, want_rets), (bname, align, "rets", first_difference(got_rets, want_rets))
        assert np.array_equal(got, want), (bname, align, "dense buffer: (offset, got, want, bytes that differ)", first_difference(got, want))


@pytest.mark.parametrize("bname", BATCHES)
def test_reader_one_byte_short(lib, oracle, bname):
    """dense_capacity one byte below offsets[n] (byte-dense): exactly the last non-empty chunk is refused with SPRINTZ_E_CORRUPT and
    leaves the poison, every other chunk is exact, the guard is untouched.  (Every drive batch ends in a non-empty chunk: an empty one
    behind it would START beyond such a capacity and be refused as well.)"""
    b, dense, offs, sizes, *_ = source(bname)
    assert len(b["chunks"][-1]) > 0
    container, ho, tables = oracle_written(oracle, bname)
    n, total_in = len(sizes), int(sizes.astype(np.int64).sum())
    assert lib.E_CORRUPT == -5
    want_offs, want, want_rets = expected_dense(b["chunks"], 1, capacity=total_in - 1)
    assert (want_rets == -5).sum() == 1 and want_rets[-1] == -5
    got, got_offs, got_sizes, got_rets = run_reader(lib, container, ho, tables, n, total_in, 1, total_in - 1, want.size)
    assert np.array_equal(got_offs, want_offs) and np.array_equal(got_sizes, sizes)
    assert np.array_equal(got_rets, want_rets), (bname, first_difference(got_rets, want_rets))
    assert np.array_equal(got, want), (bname, first_difference(got, want))


# ----------------------------------------------------------------- the shared-table Huff0 writer behind the same K1

def huf0_written(lib, oracle, bname):
    if ("huf0", bname) not in _cache:
        import torch
        b, dense, offs, sizes, d_dense, d_offs, d_sizes = source(bname)
        n, total = len(sizes), int(sizes.astype(np.int64).sum())
        bound = int(lib.huf0_bound(total, n))
        d_blocks = filled(bound + GUARD, SENT)
        d_bo = filled(8 * (n + 1) + GUARD, SENT)
        d_tmp = filled(int(lib.huf0_tmp_bytes(n)) + GUARD, SENT)
        lib.check(lib.huf0_compress_batch(d_dense.data_ptr(), d_offs.data_ptr(), d_sizes.data_ptr(), n, d_blocks.data_ptr(), d_bo.data_ptr(),
                                          d_tmp.data_ptr(), None))
        torch.cuda.synchronize()
        bo_raw = d_bo.cpu().numpy()
        assert (bo_raw[8 * (n + 1):] == SENT).all() and (d_tmp.cpu().numpy()[int(lib.huf0_tmp_bytes(n)):] == SENT).all()
        _cache["huf0", bname] = (d_blocks.cpu().numpy(), bo_raw[:8 * (n + 1)].view(np.uint64).copy())
    return _cache["huf0", bname]


@pytest.mark.parametrize("bname", BATCHES)
def test_huf0_writer_on_the_same_batches(lib, oracle, bname):
    """huf0_compress_batch writes oracle_huf0_compress_batch's blocks (every byte, nothing behind them), and the oracle's restatement
    of HUF_decompress turns every block back into its chunk"""
    b, dense, offs, sizes, *_ = source(bname)
    want, wo = oracle.huf0_compress(dense, offs, sizes)
    got, bo = huf0_written(lib, oracle, bname)
    assert np.array_equal(bo, wo), (bname, "block offsets", first_difference(bo, wo))
    assert np.array_equal(got[:want.size], want), (bname, "blocks", first_difference(got[:want.size], want))
    assert (got[want.size:] == SENT).all(), (bname, "written behind the last block")
    for c, ch in enumerate(b["chunks"]):
        blk = got[int(bo[c]):int(bo[c + 1])]
        if len(ch) == 0:
            assert blk.size == 0, (bname, c)
            continue
        back, ret = oracle.huf0_decompress(blk, len(ch))
        assert ret == len(ch) and np.array_equal(back, ch), (bname, c, ret)


def test_huf0_blocks_are_read_by_libzstd(lib, oracle):
    """the system library's own HUF_decompress reads a coded block of every drive segment that has one"""
    try:
        z = Zstd()
    except (OSError, AttributeError):
        pytest.skip("no libzstd with the HUF_* exports on this machine")
    read = 0
    for bname in BATCHES:
        b, dense, offs, sizes, *_ = source(bname)
        got, bo = huf0_written(lib, oracle, bname)
        for sname, first in b["segments"]:
            for c in range(first, min(first + hd.SEG, len(b["chunks"]))):
                ch, blk = b["chunks"][c], got[int(bo[c]):int(bo[c + 1])]
                if 1 < blk.size < len(ch) <= 128 * 1024:                     # coded, and a size HUF_compress itself would take
                    back, ret = z.huf_decompress(blk, len(ch))
                    assert ret == len(ch) and np.array_equal(back, ch), (bname, sname, c, ret)
                    read += 1
                    break
    assert read >= 20, read
