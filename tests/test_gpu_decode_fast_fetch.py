"""GPU tests (-m gpu) of how decode_fast.h FETCHES a stream.  Its read-ahead starts on the cache line a stream starts in, runs across the
gaps and chunk boundaries inside a lane group and past the group's last stream, and tops the ring up by one to three units a step.
None of that may reach a decoded byte -- whatever the container's phase against the cache lines, whatever lies between and behind the
streams, however much a step consumes -- and a change to the fetch path (ending the read-ahead with the group's last stream, fewer
requests in the common step: DESIGN_HISTORY 4.1 (i)) has these cases to pass.  So every case decodes containers BUILT BY HAND from the
oracle's streams (tests/harness.py) -- gaps, fill bytes, the container's start and the stream ends are the test's to choose -- and
compares with the oracle's decode of the same streams.  The batches are small, so SPRINTZ_OPT_LAT_CHUNKS = 0 sends them to the
lane-per-column kernels, and the dispatch counters (tests/dispatch.py) say that decode_fast.h took every one of them.

Shapes: uint16 x 8 columns, FIRE, 67 chunks (8 chunks a wavefront: the last wave holds 3), one and three chunks a lane group.
Chunk lengths: 1 280 elements = 10 group steps; 384 = 3 steps, the shortest whole number of steps the planner gives this kernel
(plan.h wants a chunk of at least half the 1 216-byte LDS carve of a lane group: 304 elements); 304 = 2 steps and a verbatim tail
of 48 elements.  Chunks of 128 and 256 elements (1 and 2 steps) are below that bound and decode on decode_kernel.h: they run here
too, against the same oracle, and the counters say which kernel took them.
"""
import os
import sys

import numpy as np
import pytest

from dispatch import ran
from harness import DTYPES
from fixtures import sz  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

NCHUNKS = 67
FAST_LENS = [1280, 384, 304]          # decode_fast.h: 10 steps / 3 steps / 2 steps + a tail
SHORT_LENS = [128, 256]               # 1 / 2 steps: below the planner's bound for decode_fast.h (module docstring)


@pytest.fixture(autouse=True)
def lane_per_column_kernels(sz, request):
    """small batches on the lane-per-column kernels, as tests/test_gpu_dispatch.py forces them; both options restored afterwards"""
    from sprintz_amd import _lib
    _lib.check(_lib.set_option(_lib.OPT_LAT_CHUNKS, 0))

    def restore():
        _lib.set_option(_lib.OPT_LAT_CHUNKS, int(os.environ.get("SPRINTZ_MI355X_LAT_CHUNKS", 2048)))
        _lib.set_option(_lib.OPT_CHUNKS_PER_GROUP, int(os.environ.get("SPRINTZ_MI355X_CHUNKS_PER_GROUP", 1)))
    request.addfinalizer(restore)


def set_chunks_per_group(k):
    from sprintz_amd import _lib
    _lib.check(_lib.set_option(_lib.OPT_CHUNKS_PER_GROUP, k))


# ------------------------------------------------------------------ data, streams and the oracle's decode (computed once per key)

_CACHE = {}


def synth(kind, esz, nchunks, rows, D, seed=123):
    from synth import synth_numpy
    name, step = {"uniform": ("uniform", 8), "walk8": ("walk", 8), "walk300": ("walk", 300), "walk2": ("walk", 2), "walkflat": ("walkflat", 8)}[kind]
    return synth_numpy(name, esz, nchunks, rows, D, seed=seed, step=step)


def make_data(kind, esz, D, chunk_len, nchunks):
    rows = chunk_len // D
    assert rows * D == chunk_len or kind == "walk8"
    if kind == "mixed":                                   # within every wave: uniform and walk8 chunks alternate
        u = synth("uniform", esz, nchunks, rows, D).reshape(nchunks, -1)
        w = synth("walk8", esz, nchunks, rows, D).reshape(nchunks, -1)
        u[1::2] = w[1::2]
        return u.reshape(-1)
    if kind == "runend":                                  # 16 rows of a walk, then the same row to the chunk's end: one run of >= 128 blocks
        x = synth("walk8", esz, nchunks, rows, D).reshape(nchunks, rows, D).copy()
        x[:, 16:] = x[:, 15:16]
        return x.reshape(-1)
    if rows * D != chunk_len:                             # chunks that do not hold whole rows: one series, cut
        return synth(kind, esz, 1, -(-nchunks * chunk_len // D), D)[: nchunks * chunk_len].copy()
    return synth(kind, esz, nchunks, rows, D)


def prepared(oracle, codec, kind, esz, D, chunk_len, nchunks, total_len=None):
    """-> (streams, want, want_rets): the oracle's stream of every chunk and the oracle's decode of it"""
    key = (codec, kind, esz, D, chunk_len, nchunks, total_len)
    if key not in _CACHE:
        data = make_data(kind, esz, D, chunk_len, nchunks)
        if total_len is not None:
            data = data[:total_len]
        streams = oracle.compress_chunks(codec, data, chunk_len, D)
        assert len(streams) == nchunks
        want = np.zeros(nchunks * chunk_len, DTYPES[esz])
        rets = np.zeros(nchunks, np.int64)
        for c, s in enumerate(streams):
            o, r = oracle.decompress(codec, s, esz, chunk_len)
            assert 0 <= r <= chunk_len
            want[c * chunk_len:c * chunk_len + r] = o[:r]
            rets[c] = r
        assert np.array_equal(want[:data.size], data) and rets.sum() == data.size       # the oracle round-trips its own streams
        want.setflags(write=False)
        rets.setflags(write=False)
        _CACHE[key] = (streams, want, rets)
    return _CACHE[key]


def lay_out(streams, gaps=None, align=1, fill=0, lead=0, starts=None):
    """a container by hand: stream c at offsets[c], offsets[c + 1] = its end + gaps[c] (or rounded up to `align`), `fill` in every byte
    that belongs to no stream -- the READ_SLACK bytes behind the last one included.  starts: explicit offsets instead.
    -> (bytes, offsets[n + 1])"""
    from sprintz_amd import _lib
    n = len(streams)
    offs = np.zeros(n + 1, np.int64)
    pos = lead
    for c, s in enumerate(streams):
        if starts is not None:
            assert starts[c] >= pos
            pos = int(starts[c])
        offs[c] = pos
        pos += s.size
        if gaps is not None:
            pos += int(gaps[c])
        pos = -(-pos // align) * align
    offs[n] = pos
    comp = np.full(pos + _lib.READ_SLACK, fill, np.uint8)
    for c, s in enumerate(streams):
        comp[offs[c]:offs[c] + s.size] = s
    return comp, offs


def decode(sz, codec, esz, D, chunk_len, comp_t, offs, nchunks, family="dec_fast"):
    """one decompress_batch call on `family` (asserted) -> (out, rets) on the host; the output's guard elements checked"""
    import torch
    cd = sz.ChunkedCodec(codec, esz, D, chunk_len, device="cuda:0")
    n = nchunks * chunk_len
    obuf = torch.full((n + 64,), 0x5A, dtype=torch.int8 if esz == 1 else torch.int16, device="cuda:0").view(cd.dtype)
    rets = torch.full((nchunks,), -77, dtype=torch.int64, device="cuda:0")
    offs_t = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).cuda()
    with ran(only=[family], **{family: 1}):
        cd.decompress_into(comp_t, offs_t, nchunks, obuf[:n], rets)
    o = obuf.cpu().numpy().view(DTYPES[esz])
    assert (o[n:] == 0x5A).all(), "wrote behind the output"
    return o[:n], rets.cpu().numpy()


def check(out, rets, want, want_rets, chunk_len, tag=""):
    assert np.array_equal(rets, want_rets), (tag, rets[:16], want_rets[:16])
    for c in np.flatnonzero(want_rets < chunk_len):       # a short chunk: only what it holds is compared
        out = out.copy()
        out[c * chunk_len + want_rets[c]:(c + 1) * chunk_len] = 0
    assert np.array_equal(out, want), (tag, "first difference at element", int(np.flatnonzero(out != want)[0]))


def on_device(comp):
    import torch
    return torch.from_numpy(comp).cuda()


# ------------------------------------------------------------------ 1. bytes outside a stream do not matter

GAPS = list(range(17)) + [4096]        # 0 .. 16: stepped over; 4 096: the read-ahead starts again at that chunk


@pytest.mark.parametrize("cpg", [1, 3])
@pytest.mark.parametrize("chunk_len", FAST_LENS + SHORT_LENS)
def test_bytes_outside_a_stream_do_not_matter(sz, oracle, chunk_len, cpg):
    """the same streams in a container padded with zeros and in one with 0xA5 in every gap and behind the last stream: what the
    read-ahead fetched from a gap, from the next group's streams or from behind the container reaches no output byte"""
    family = "dec_fast" if chunk_len in FAST_LENS else "dec_generic"
    streams, want, want_rets = prepared(oracle, "xff", "walk8", 2, 8, chunk_len, NCHUNKS)
    gaps = [GAPS[c % len(GAPS)] for c in range(NCHUNKS)]
    set_chunks_per_group(cpg)
    got = []
    for fill in (0, 0xA5):
        comp, offs = lay_out(streams, gaps=gaps, fill=fill)
        out, rets = decode(sz, "xff", 2, 8, chunk_len, on_device(comp), offs, NCHUNKS, family)
        check(out, rets, want, want_rets, chunk_len, f"fill {fill:#x}")
        got.append((out, rets))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


# ------------------------------------------------------------------ 2. every line phase

@pytest.mark.parametrize("cpg", [1, 3])
@pytest.mark.parametrize("align", [1, 16])
@pytest.mark.parametrize("delta", [0, 1, 15])
def test_every_phase_of_the_container_against_the_cache_lines(sz, oracle, delta, align, cpg):
    """the container starts 16 k + delta bytes into an allocation, k = 0 .. 7: its first stream anywhere in a 128-byte line -- at byte 0
    of the allocation too, where rounding a load address down to the line would leave the container -- and its last stream ends
    READ_SLACK bytes before the allocation's end.  Byte-dense and 16-byte aligned layouts; 0xA5 around the container."""
    import torch
    from sprintz_amd import _lib
    chunk_len = 1280
    streams, want, want_rets = prepared(oracle, "xff", "walk8", 2, 8, chunk_len, NCHUNKS)
    comp, offs = lay_out(streams, align=align, fill=0xA5)
    total = int(offs[-1])
    assert comp.size == total + _lib.READ_SLACK
    set_chunks_per_group(cpg)
    for k in range(8):
        start = 16 * k + delta
        buf = torch.full((start + comp.size,), 0xA5, dtype=torch.uint8, device="cuda:0")     # ends READ_SLACK behind the last stream
        assert buf.data_ptr() % 128 == 0
        buf[start:] = torch.from_numpy(comp).cuda()
        out, rets = decode(sz, "xff", 2, 8, chunk_len, buf[start:], offs, NCHUNKS)
        check(out, rets, want, want_rets, chunk_len, f"start {start}")
        del buf


# ------------------------------------------------------------------ 3. more than one unit a step

@pytest.mark.parametrize("cpg", [1, 3])
@pytest.mark.parametrize("kind,chunk_len", [("uniform", 1280), ("walk300", 1280), ("mixed", 1280), ("walkflat", 5120), ("runend", 8576),
                                            ("uniform", 384), ("mixed", 304)])
def test_steps_that_take_more_than_one_unit(sz, oracle, kind, chunk_len, cpg):
    """incompressible data takes ~268 bytes a step and walk +-300 ~170, so that every step wants a second or third unit; uniform and
    walk +-8 chunks alternating inside a wave leave the eight groups at different ring phases with only some of them wanting more;
    flat spans bring run slots, and a chunk that ends in ONE run of 132 blocks a two-byte run length and a run that ends the stream"""
    streams, want, want_rets = prepared(oracle, "xff", kind, 2, 8, chunk_len, NCHUNKS)
    if kind == "runend":
        assert all(s.size < 600 for s in streams)                       # 16 rows of payload and the run, not 1 072 rows of payload
    comp, offs = lay_out(streams, align=16, fill=0xA5)
    set_chunks_per_group(cpg)
    out, rets = decode(sz, "xff", 2, 8, chunk_len, on_device(comp), offs, NCHUNKS)
    check(out, rets, want, want_rets, chunk_len, kind)


# ------------------------------------------------------------------ 4. stream ends

@pytest.mark.parametrize("cpg", [1, 3])
@pytest.mark.parametrize("align", [1, 16])
def test_a_verbatim_tail_then_the_next_chunk(sz, oracle, align, cpg):
    """1 320 elements = 10 groups and 40 verbatim elements: the tail is copied from behind the last group, the cursor is then not at
    the next stream, and the next chunk of the lane group (three a group) starts from a fresh prime"""
    chunk_len = 1320
    streams, want, want_rets = prepared(oracle, "xff", "walk8", 2, 8, chunk_len, NCHUNKS)
    comp, offs = lay_out(streams, align=align, fill=0xA5)
    set_chunks_per_group(cpg)
    out, rets = decode(sz, "xff", 2, 8, chunk_len, on_device(comp), offs, NCHUNKS)
    check(out, rets, want, want_rets, chunk_len)


@pytest.mark.parametrize("cpg", [1, 3])
@pytest.mark.parametrize("last", [24, 640, 1272])
def test_a_short_last_chunk(sz, oracle, last, cpg):
    """the batch's last chunk holds fewer elements than the others; 24 elements are a stream of 56 bytes -- shorter than one 128-byte unit"""
    chunk_len = 1280
    total = (NCHUNKS - 1) * chunk_len + last
    streams, want, want_rets = prepared(oracle, "xff", "walk8", 2, 8, chunk_len, NCHUNKS, total_len=total)
    if last == 24:
        assert streams[-1].size == 8 + 2 * 24
    assert want_rets[-1] == last
    comp, offs = lay_out(streams, align=1, fill=0xA5)
    set_chunks_per_group(cpg)
    out, rets = decode(sz, "xff", 2, 8, chunk_len, on_device(comp), offs, NCHUNKS)
    check(out, rets, want, want_rets, chunk_len)


# bytes between a stream's end and the next 128-byte line boundary.  (A stream of walk +-8 is 8 bytes of header and whole 8-byte payload
# rows -- 960 or 968 bytes a chunk of 1 280 elements with seed 123 -- so no seed ends one 1, 15 or 17 bytes before a line from a
# line-aligned start: the container places every stream so that it ENDS there instead.)
LINE_ENDS = [0, 1, 15, 16, 17, 127]


@pytest.mark.parametrize("cpg", [1, 3])
def test_streams_that_end_at_every_distance_from_a_line_boundary(sz, oracle, cpg):
    chunk_len = 1280
    streams, want, want_rets = prepared(oracle, "xff", "walk8", 2, 8, chunk_len, NCHUNKS)
    assert {s.size for s in streams} <= {960, 968, 976}, sorted({s.size for s in streams})
    starts, pos = [], 0
    for c, s in enumerate(streams):
        d = LINE_ENDS[c % len(LINE_ENDS)]
        end = -(-(pos + s.size + d) // 128) * 128 - d                   # the first such end the stream fits in front of
        starts.append(end - s.size)
        pos = end
    comp, offs = lay_out(streams, starts=starts, fill=0xA5)
    for c, s in enumerate(streams):
        assert (128 - (offs[c] + s.size) % 128) % 128 == LINE_ENDS[c % len(LINE_ENDS)]
    t = on_device(comp)
    assert t.data_ptr() % 128 == 0
    set_chunks_per_group(cpg)
    out, rets = decode(sz, "xff", 2, 8, chunk_len, t, offs, NCHUNKS)
    check(out, rets, want, want_rets, chunk_len)


# ------------------------------------------------------------------ 5. the template's other instantiations

@pytest.mark.parametrize("cpg", [1, 3])
@pytest.mark.parametrize("codec,esz,D,chunk_len,nchunks,kind", [
    ("delta", 1, 80, 5120, 9, "walk2"),         # SPLIT: 32 lanes x (a pair + a single column)
    ("xff", 1, 16, 2048, 19, "walk2"),          # one 8-bit column a lane, 16 lanes: a unit of 256 bytes
    ("xff", 2, 3, 1536, 35, "walk8"),           # 4 lanes a chunk: a unit of 64 bytes, half a line
    ("xff", 2, 8, 1280, 19, "uniform"),
], ids=["u8x80_delta_split", "u8x16_fire", "u16x3", "u16x8_uniform_19"])
def test_other_instantiations(sz, oracle, codec, esz, D, chunk_len, nchunks, kind, cpg):
    streams, want, want_rets = prepared(oracle, codec, kind, esz, D, chunk_len, nchunks)
    set_chunks_per_group(cpg)
    for align, lead in ((16, 0), (1, 0), (1, 37)):
        comp, offs = lay_out(streams, align=align, fill=0xA5, lead=lead)
        out, rets = decode(sz, codec, esz, D, chunk_len, on_device(comp), offs, nchunks)
        check(out, rets, want, want_rets, chunk_len, f"align {align} lead {lead}")


def hand_batch(sz, streams, esz, D, chunk_len, align=16, fill=0xA5):
    import torch
    comp, offs = lay_out(streams, align=align, fill=fill)
    sizes = torch.tensor([s.size for s in streams], dtype=torch.int32, device="cuda:0")
    return sz.codec.CompressedBatch(on_device(comp), torch.from_numpy(offs).cuda(), sizes, len(streams), len(streams) * chunk_len, chunk_len, D)


def test_column_major_destination(sz, oracle):
    """uint16 x 32 columns, 160 rows a chunk, 9 chunks, every column's samples contiguous in the output"""
    D, R, n = 32, 160, 9
    streams, want, _ = prepared(oracle, "xff", "walk8", 2, D, R * D, n)
    cd = sz.ChunkedCodec("xff", 2, D, R * D, device="cuda:0")
    batch = hand_batch(sz, streams, 2, D, R * D)
    with ran(only=["dec_fast"], dec_fast=1):
        cols = cd.decompress_colmajor(batch)
    assert np.array_equal(cols.cpu().numpy().view(np.uint16), want.reshape(n * R, D).T)


def test_gather_rows_that_start_mid_chunk_and_end_with_a_chunk(sz, oracle):
    """three ranges from row 37 of a chunk to the last row of the NEXT chunk: the first piece starts mid-chunk, the last one ends with
    its chunk's -- and its stream's -- last group; the batch's last chunk among them"""
    D, R, n = 8, 160, NCHUNKS
    streams, want, _ = prepared(oracle, "xff", "walk8", 2, D, R * D, n)
    cd = sz.ChunkedCodec("xff", 2, D, R * D, device="cuda:0")
    rows = 2 * R - 37
    starts = np.array([37, 5 * R + 37, (n - 2) * R + 37], np.int64)
    x = want.reshape(n * R, D)
    for align in (16, 1):
        batch = hand_batch(sz, streams, 2, D, R * D, align=align)
        with ran(only=["gather_fast"], gather_fast=1):
            got = cd.gather_rows(batch, starts, rows)
        assert np.array_equal(got.cpu().numpy().view(np.uint16), np.stack([x[s:s + rows] for s in starts])), align


def test_windowed_query(sz, oracle):
    """per-window min / max / sum of 32-row windows, 160 rows a chunk, from the same hand-built container"""
    D, R, n, W = 8, 160, NCHUNKS, 32
    streams, want, _ = prepared(oracle, "xff", "walk8", 2, D, R * D, n)
    cd = sz.ChunkedCodec("xff", 2, D, R * D, device="cuda:0")
    batch = hand_batch(sz, streams, 2, D, R * D, align=1)
    with ran(only=["dec_fast"], dec_fast=1):
        res = cd.query_windows(batch, W, per_chunk=True)
    x = want.reshape(n, R // W, W, D).astype(np.int64)
    assert np.array_equal(res["min"].cpu().numpy().view(np.uint16), x.min(axis=2))
    assert np.array_equal(res["max"].cpu().numpy().view(np.uint16), x.max(axis=2))
    assert np.array_equal(res["sum"].cpu().numpy(), x.sum(axis=2))


# ------------------------------------------------------------------ 6. damaged streams

@pytest.mark.parametrize("cpg", [1, 3])
@pytest.mark.parametrize("damage", ["cut1", "cut_unit", "groups"])
def test_damaged_streams_are_reported_and_their_neighbours_decode(sz, oracle, damage, cpg):
    """chunks 5, 30 and the last one damaged: cut short by one byte, by one unit of 128 bytes -- the next stream follows at once in the
    byte-dense container -- or with a header that announces more groups than the stream can hold (which bounds the group loop: the call
    returns).  Those chunks report SPRINTZ_E_CORRUPT; every other chunk decodes as the oracle does."""
    from sprintz_amd import _lib
    chunk_len = 1280
    streams, want, want_rets = prepared(oracle, "xff", "walk8", 2, 8, chunk_len, NCHUNKS)
    bad = [5, 30, NCHUNKS - 1]
    streams = [s.copy() for s in streams]
    for c in bad:
        if damage == "cut1":
            streams[c] = streams[c][:-1]
        elif damage == "cut_unit":
            streams[c] = streams[c][:-128]
        else:
            streams[c][:4] = np.frombuffer(np.uint32(streams[c].size).tobytes(), np.uint8)       # ngroups: 10 bytes a group would not fit
    comp, offs = lay_out(streams, align=1, fill=0xA5)
    set_chunks_per_group(cpg)
    out, rets = decode(sz, "xff", 2, 8, chunk_len, on_device(comp), offs, NCHUNKS)
    good = np.setdiff1d(np.arange(NCHUNKS), bad)
    assert (rets[bad] == _lib.E_CORRUPT).all(), rets[bad]
    assert np.array_equal(rets[good], want_rets[good])
    o, w = out.reshape(NCHUNKS, chunk_len), want.reshape(NCHUNKS, chunk_len)
    assert np.array_equal(o[good], w[good])
