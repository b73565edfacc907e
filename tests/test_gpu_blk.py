"""GPU tests (-m gpu) of the round-6 delta kernels (csrc/encode_blk.h, decode_blk.h, decode_row.h; SPRINTZ_OPT_BLK_CHUNKS, SPRINTZ_OPT_BLK_KERNELS):
every shape family they take, batched through the C-ABI, against the oracle -- stream bytes, sizes, return values, samples.  The general
parity modules run with these kernels switched on too (tests/conftest.py: decode_path "blk").

Equal bytes do not show which kernel wrote them -- every family writes the same, and a launch site that refuses a shape falls through to an
older kernel without a word.  So every call here also asserts the kernel family it was served by, from the library's dispatch counters
(tests/dispatch.py): SHAPES states, per shape and per `path`, the encoder and the decoder the shape must land on, derived from the "Shapes"
paragraphs of the kernels' headers and the option's text in sprintz_mi355x.h -- or, where a kernel does not take the shape, `falls through:`
and why, and then that NO round-6 family ran.  path "old" must show none of them anywhere."""
import numpy as np
import pytest

from dispatch import OLD_DECODERS, OLD_ENCODERS, ROUND6, ran
from harness import DTYPES, gen_walk
from fixtures import sz  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["blk", "row", "old"])
def path(request):
    """every test on the block-parallel kernels ("blk": encode_blk + decode_blk + encode_blk_uni; "row": encode_blk + the piece-sequential
    decoder decode_row.h) and, as a control, on the kernels they replace (same bytes)"""
    import os
    from sprintz_amd import _lib
    _lib.check(_lib.set_option(_lib.OPT_LAT_CHUNKS, 0))
    _lib.check(_lib.set_option(_lib.OPT_BLK_CHUNKS, 0 if request.param == "old" else 1))
    _lib.check(_lib.set_option(_lib.OPT_BLK_KERNELS, 25 if request.param == "row" else 7))
    yield request.param
    _lib.set_option(_lib.OPT_LAT_CHUNKS, int(os.environ.get("SPRINTZ_MI355X_LAT_CHUNKS", 2048)))
    _lib.set_option(_lib.OPT_BLK_CHUNKS, int(os.environ.get("SPRINTZ_MI355X_BLK_CHUNKS", 2049)))
    _lib.set_option(_lib.OPT_BLK_KERNELS, int(os.environ.get("SPRINTZ_MI355X_BLK_KERNELS", 9)))


def make_data(kind, rng, n, ndims, esz):
    if kind == "walk":
        return gen_walk(rng, n, ndims, esz, 3)
    if kind == "walk_flat":                                   # flat spans: runs inside and across groups, runs that end a chunk
        return gen_walk(rng, n, ndims, esz, 5, flat_every=2)
    if kind == "zeros":
        return np.zeros(n, DTYPES[esz])
    if kind == "const_cols":                                  # all-zero deltas after the first row: one long run per chunk
        return np.tile(rng.integers(0, 1 << (8 * esz), ndims).astype(DTYPES[esz]), (n + ndims - 1) // ndims)[:n]
    if kind == "noise":                                       # every width at its maximum
        return rng.integers(0, 1 << (8 * esz), n).astype(DTYPES[esz])
    if kind == "mixed":                                       # per column a different step size: every width 0 .. W in one row
        rows = (n + ndims - 1) // ndims
        amp = (1 << (rng.integers(0, 8 * esz + 1, ndims))) >> 1
        steps = rng.integers(-1, 2, (rows, ndims)) * amp[None, :]
        steps[(np.arange(rows) // 24) % 3 == 1] = 0
        return np.mod(np.cumsum(steps, axis=0), 1 << (8 * esz)).astype(DTYPES[esz]).ravel()[:n]
    raise ValueError(kind)


# why a shape is not on a round-6 kernel under a path that asks for it
COLS8 = "falls through: decode_blk.h walks a group header on 16 lanes of 10 fields: 8-bit rows of at most 80 columns"
COLS16 = "falls through: decode_blk.h walks a group header on 16 lanes of 8 fields: 16-bit rows of at most 64 columns"
COLS8_SHORT = COLS8 + "; and chunks of at least 32 rows"
PIECES = "falls through: encode_blk.h and decode_blk.h take rows of whole 16-byte pieces"
LOWDIM = "falls through: the low-dim layout has no round-6 decoder (decode_uni.h)"
MASK25 = "falls through: mask 25 leaves bit 2 (encode_blk_uni) off"

SHAPES = [
    # esz, ndims, chunk_len (elements), nchunks, ragged last chunk (elements short of a full one);
    # then the kernel family: path "blk" (mask 7) encode, decode; path "row" (mask 25) encode, decode
    (1, 80, 10240, 37, 0, "enc_blk", "dec_blk", "enc_blk", "dec_row"),            # BASELINE config 3 at 10 KB
    (1, 80, 10240, 5, 3000, "enc_blk", "dec_blk", "enc_blk", "dec_row"),
    (1, 16, 2048, 64, 0, "enc_blk", "dec_blk", "enc_blk", "dec_row"),
    (1, 16, 16 * 16 * 3 + 32, 19, 48, "enc_blk", "dec_blk", "enc_blk", "dec_row"),  # chunk not a whole number of blocks
    (1, 32, 4096, 33, 0, "enc_blk", "dec_blk", "enc_blk", "dec_row"),
    (1, 48, 48 * 40, 21, 0, "enc_blk", "dec_blk", "enc_blk", "dec_row"),
    (1, 64, 8192, 17, 64 * 5, "enc_blk", "dec_blk", "enc_blk", "dec_row"),
    (1, 96, 96 * 24, 13, 0, "enc_blk", COLS8_SHORT, "enc_blk", "dec_row"),
    (1, 128, 128 * 16, 11, 0, "enc_blk", COLS8_SHORT, "enc_blk", "dec_row"),        # exactly one group a chunk
    (1, 256, 256 * 16 * 2, 6, 0, "enc_blk", COLS8, "enc_blk", "dec_row"),
    (2, 8, 5120, 70, 0, "enc_blk", "dec_blk", "enc_blk", "dec_row"),              # the headline shape on the delta codec
    (2, 8, 5120, 9, 1000, "enc_blk", "dec_blk", "enc_blk", "dec_row"),
    (2, 8, 8 * 16 * 2 + 8, 40, 0, "enc_blk", "dec_blk", "enc_blk", "dec_row"),
    (2, 16, 4096, 21, 0, "enc_blk", "dec_blk", "enc_blk", "dec_row"),
    (2, 24, 24 * 56, 15, 24 * 3, "enc_blk", "dec_blk", "enc_blk", "dec_row"),
    (2, 40, 40 * 128, 9, 0, "enc_blk", "dec_blk", "enc_blk", "dec_row"),
    (2, 64, 64 * 32, 9, 0, "enc_blk", "dec_blk", "enc_blk", "dec_row"),
    (2, 80, 80 * 64, 7, 0, "enc_blk", COLS16, "enc_blk", "dec_row"),
    (2, 128, 128 * 16, 5, 0, "enc_blk", COLS16 + "; and chunks of at least 32 rows", "enc_blk", "dec_row"),
    # rows of whole dwords that are not whole 16-byte pieces: the column-group-sequential decoder alone (decode_row.h)
    (1, 12, 12 * 40, 50, 0, PIECES, PIECES, PIECES, "dec_row"),
    (1, 20, 20 * 64, 31, 20 * 7, PIECES, PIECES, PIECES, "dec_row"),
    (1, 8, 1024, 90, 0, PIECES, PIECES, PIECES, "dec_row"),
    (2, 6, 6 * 80, 41, 0, PIECES, PIECES, PIECES, "dec_row"),
    (2, 10, 10 * 48, 33, 0, PIECES, PIECES, PIECES, "dec_row"),
    (2, 4, 2048, 60, 0, PIECES, PIECES, PIECES, "dec_row"),
    # univariate streams of the low-dim layout (encode_blk_uni_kernel)
    (1, 1, 1024, 300, 0, "enc_blk_uni", LOWDIM, MASK25, LOWDIM),             # BASELINE config 1
    (1, 1, 1024, 67, 500, "enc_blk_uni", LOWDIM, MASK25, LOWDIM),
    (1, 1, 4096, 40, 16, "enc_blk_uni", LOWDIM, MASK25, LOWDIM),
    (1, 1, 272, 90, 0, "enc_blk_uni", LOWDIM, MASK25, LOWDIM),
    (1, 1, 128, 90, 0, "enc_blk_uni", LOWDIM, MASK25, LOWDIM),               # the shortest chunk that holds a group
    (1, 1, 112, 33, 0, "enc_blk_uni", LOWDIM, MASK25, LOWDIM),               # below 128 elements: no group, all of it the tail -- still seven 16-byte tasks of the kernel
    (2, 1, 512, 150, 0, "enc_blk_uni", LOWDIM, MASK25, LOWDIM),
    (2, 1, 2048, 40, 200, "enc_blk_uni", LOWDIM, MASK25, LOWDIM),
    (2, 1, 200, 77, 0, "enc_blk_uni", LOWDIM, MASK25, LOWDIM),
]
FAMILY = {s[:5]: {"blk": s[5:7], "row": s[7:9]} for s in SHAPES}
assert len(FAMILY) == len(SHAPES)


def encodes_on(path, fam):
    """the dispatch assertion around a compress() call whose container is 16-byte aligned: the encoder, then how the container was built"""
    if path == "old" or fam.startswith("falls through:"):
        return ran(never=ROUND6, one_of=OLD_ENCODERS, only=OLD_ENCODERS + ("dense_fused", "dense_compact"), what=f"path {path}: {fam}")
    return ran(only=[fam, "dense_compact"], what=f"path {path}", **{fam: 1, "dense_compact": 1})


def decodes_on(path, fam):
    if path == "old" or fam.startswith("falls through:"):
        return ran(never=ROUND6, one_of=OLD_DECODERS, only=OLD_DECODERS, what=f"path {path}: {fam}")
    return ran(only=[fam], what=f"path {path}", **{fam: 1})


@pytest.mark.parametrize("kind", ["walk", "walk_flat", "zeros", "const_cols", "noise", "mixed"])
@pytest.mark.parametrize("esz,ndims,chunk_len,nchunks,short", [s[:5] for s in SHAPES])
def test_delta_batches_match_the_oracle(sz, oracle, path, kind, esz, ndims, chunk_len, nchunks, short):
    import torch
    enc_fam, dec_fam = FAMILY[(esz, ndims, chunk_len, nchunks, short)].get(path, ("old", "old"))
    rng = np.random.default_rng(1000 * ndims + chunk_len + esz)
    n = nchunks * chunk_len - short
    data = make_data(kind, rng, n, ndims, esz)
    cd = sz.ChunkedCodec("delta", esz, ndims, chunk_len, device="cuda:0")
    t = torch.from_numpy(data.view(np.int8 if esz == 1 else np.int16)).cuda().view(cd.dtype)
    with encodes_on(path, enc_fam):
        batch = cd.compress(t)
    sizes, offs, comp = batch.sizes.cpu().numpy(), batch.offsets.cpu().numpy(), batch.data.cpu().numpy()
    for c in range(nchunks):
        want, wret = oracle.compress("delta", data[c * chunk_len:(c + 1) * chunk_len], ndims)
        assert sizes[c] == want.size, (path, kind, c, int(sizes[c]), want.size)
        got = comp[offs[c]:offs[c] + sizes[c]]
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError((path, kind, "chunk", c, "first differing stream bytes", bad[:6].tolist(), "of", want.size,
                                  got[bad[:6]].tolist(), want[bad[:6]].tolist()))
    rets = torch.empty(nchunks, dtype=torch.int64, device="cuda:0")
    with decodes_on(path, dec_fam):
        out = cd.decompress(batch, rets=rets)
    out = out.cpu().numpy().view(DTYPES[esz])
    assert np.array_equal(out[:n], data), (path, kind)
    r = rets.cpu().numpy()
    assert (r[:-1] == chunk_len).all() and r[-1] == chunk_len - short, (path, kind, r[-3:])


@pytest.mark.parametrize("esz,ndims,chunk_len", [(1, 80, 10240), (2, 8, 5120), (1, 16, 1024), (1, 1, 1024), (2, 1, 1024)])
def test_a_large_batch_takes_the_new_kernels_by_default(sz, oracle, esz, ndims, chunk_len):
    """default options, more chunks than SPRINTZ_OPT_BLK_CHUNKS' default: bytes against the oracle on every chunk -- and the kernels of the
    default mask 9 (encode_blk; decode_row where it measured faster: 8-bit rows of at least 8 dwords) where the test's name says so"""
    import torch
    enc_fam, dec_fam = {
        (1, 80, 10240): ("enc_blk", "dec_row"),
        (2, 8, 5120): ("enc_blk", "dec_fast"),        # 16-bit elements: decode_row.h did not win, decode_blk.h (bit 1) is off -- the lane-per-column kernel
        (1, 16, 1024): ("enc_blk", "dec_fast"),       # 4 dwords a row < 8: likewise
        # bit 2 (encode_blk_uni) is off by default: the lane-per-chunk kernels of the low-dim layout (encode_uni.h, decode_uni.h)
        (1, 1, 1024): ("enc_uni", "dec_uni"),
        (2, 1, 1024): ("enc_uni", "dec_uni"),
    }[(esz, ndims, chunk_len)]
    nchunks = 5000
    rng = np.random.default_rng(7)
    data = gen_walk(rng, nchunks * chunk_len, ndims, esz, 4, flat_every=5)
    cd = sz.ChunkedCodec("delta", esz, ndims, chunk_len, device="cuda:0")
    t = torch.from_numpy(data.view(np.int8 if esz == 1 else np.int16)).cuda().view(cd.dtype)
    with ran(only=[enc_fam, "dense_compact"], **{enc_fam: 1, "dense_compact": 1}):
        batch = cd.compress(t)
    sizes, offs, comp = batch.sizes.cpu().numpy(), batch.offsets.cpu().numpy(), batch.data.cpu().numpy()
    want, stride, wsizes = oracle.compress_chunks_mt("delta", data, chunk_len, ndims)
    assert np.array_equal(sizes, wsizes)
    for c in range(nchunks):
        assert np.array_equal(comp[offs[c]:offs[c] + sizes[c]], want[c * stride:c * stride + sizes[c]]), c
    with ran(only=[dec_fam], **{dec_fam: 1}):
        out = cd.decompress(batch)
    assert np.array_equal(out.cpu().numpy().view(DTYPES[esz]), data)


@pytest.mark.parametrize("esz,ndims,chunk_len,nchunks", [(1, 80, 10240, 23), (2, 8, 5120, 41), (1, 16, 2048, 50), (2, 40, 40 * 64, 17)])
def test_byte_dense_containers(sz, oracle, path, esz, ndims, chunk_len, nchunks):
    """a container whose streams start at ANY byte (sprintz_mi355x_compact with align = 1): the block-parallel decoder stages a stream from the
    16-byte piece that holds its first byte and carries the phase through every bit address"""
    import torch
    rng = np.random.default_rng(31)
    data = gen_walk(rng, nchunks * chunk_len, ndims, esz, 6, flat_every=3)
    cd = sz.ChunkedCodec("delta", esz, ndims, chunk_len, device="cuda:0", align=1)
    t = torch.from_numpy(data.view(np.int8 if esz == 1 else np.int16)).cuda().view(cd.dtype)
    # (all four shapes have rows of whole 16-byte pieces, at least 32 rows a chunk and at most 80 / 64 columns: every round-6 kernel takes them)
    with ran(never=ROUND6, one_of=OLD_ENCODERS) if path == "old" else ran(enc_blk=1, dense_compact=1, only=["enc_blk", "dense_compact"]):
        batch = cd.compress(t)
    offs, sizes, comp = batch.offsets.cpu().numpy(), batch.sizes.cpu().numpy(), batch.data.cpu().numpy()
    assert (np.diff(offs) == sizes).all() and (offs % 16 != 0).any()
    for c in range(nchunks):
        want, _ = oracle.compress("delta", data[c * chunk_len:(c + 1) * chunk_len], ndims)
        assert np.array_equal(comp[offs[c]:offs[c + 1]], want), (path, c)
    rets = torch.empty(nchunks, dtype=torch.int64, device="cuda:0")
    with decodes_on(path, {"blk": "dec_blk", "row": "dec_row", "old": "old"}[path]):
        out = cd.decompress(batch, rets=rets)
    out = out.cpu().numpy().view(DTYPES[esz])
    assert np.array_equal(out, data), path
    assert (rets.cpu().numpy() == chunk_len).all()


@pytest.mark.parametrize("esz,ndims,chunk_len,nchunks", [(1, 80, 10240, 40), (2, 8, 5120, 64), (1, 16, 2048, 70), (2, 40, 40 * 64, 24)])
def test_damaged_streams_stay_inside_their_chunk(sz, path, esz, ndims, chunk_len, nchunks):
    """bit-flipped / zeroed / all-ones / header-damaged streams through the new decoders: they terminate, write nothing outside their
    chunk's slot and report SPRINTZ_E_CORRUPT or a count within the chunk"""
    import torch
    rng = np.random.default_rng(77)
    data = gen_walk(rng, nchunks * chunk_len, ndims, esz, 8, flat_every=4)
    cd = sz.ChunkedCodec("delta", esz, ndims, chunk_len, device="cuda:0")
    batch = cd.compress(torch.from_numpy(data.view(np.int8 if esz == 1 else np.int16)).cuda().view(cd.dtype))
    comp0 = batch.data.cpu().numpy().copy()
    offs = batch.offsets.cpu().numpy()
    for trial in range(7):
        comp = comp0.copy()
        if trial == 0:
            for c in range(nchunks):
                comp[offs[c]:offs[c] + 4] = 0xFF
        elif trial == 1:
            comp[:] = 0
        elif trial == 2:
            comp[:] = 0xFF
        elif trial == 3:                                     # truncated: every stream's tail zeroed
            for c in range(nchunks):
                comp[(offs[c] + offs[c + 1]) // 2:offs[c + 1]] = 0
        else:
            idx = rng.integers(0, comp.size, comp.size // 50)
            comp[idx] ^= rng.integers(1, 256, idx.size).astype(np.uint8)
        guard = 4096
        out = torch.full((nchunks * chunk_len + guard,), 0x5A, dtype=torch.int16 if esz == 2 else torch.int8, device="cuda:0")
        rets = torch.zeros(nchunks, dtype=torch.int64, device="cuda:0")
        with decodes_on(path, {"blk": "dec_blk", "row": "dec_row", "old": "old"}[path]):          # (the shapes of the byte-dense test: every round-6 decoder takes them)
            cd.decompress_into(torch.from_numpy(comp).cuda(), batch.offsets, nchunks, out, rets)
        torch.cuda.synchronize()
        r = rets.cpu().numpy()
        assert ((r == sz._lib.E_CORRUPT) | ((r >= 0) & (r <= chunk_len))).all(), (path, trial, r[:8])
        assert (out[nchunks * chunk_len:].cpu().numpy() == 0x5A).all(), (path, trial)
