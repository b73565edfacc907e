"""GPU tests (-m gpu): the column-major kernels (BASELINE config 5) driven through runs, seams and reach.

decode_fast.h with CM = true stages four blocks of every column in LDS and flushes them on every second step, with a leftover flush for an
odd step count, a reset at the chunk loop's seam and run blocks that bypass the stage; with two and four columns a lane it holds the blocks
in registers instead.  encode_fast.h and encode_wide.h with CM = true load bursts of four blocks of a column.  decode_kernel.h and
encode_kernel.h take everything else.  Here: the run drive and the FIRE drive transposed (tests/rle_drive.py, tests/fire_drive.py), every lane
mapping, the parity of the steps with every short end, strides and alignments at the planner's edges, damaged chunks, the 32-bit reach of
both sides, side streams and empty calls.

Every comparison is exact: the expected streams are the oracle's for the row-major flattening, the expected matrix is the input, and no decode
by the library serves as an expectation.  Every call runs through tests/colmajor_runner.py on sentinel-filled buffers, whose checkers look at
the WHOLE destination, at every return value and at the kernel family that ran -- the planner's answer for the call, and the literal of
colmajor_runner's tables, which tests/test_colmajor_cpu.py replays through the planner without a device."""
import numpy as np
import pytest

import colmajor_runner as cr
import rle_drive as rd
from drive_tables import FIRE_SHAPES, batch_of, oracle_batch
from fixtures import sz  # noqa: F401  (fixtures)
from harness import DTYPES
from streams import fire_batch_of, truncated_batch

pytestmark = pytest.mark.gpu


def encode_legs(sz, oracle, codec, rows, R, legs, tag, cs=None, **kw):
    """every leg's streams, return values and family; -> the first leg's container"""
    own = None
    for pair, no_fast, family in legs:
        res = cr.encode(sz, rows, codec, R, cs=cs, pair=pair, no_fast=no_fast, **kw)
        cr.check_encode(res, oracle, codec, rows, tag + (family,))
        assert res.family == family, (tag, "the planner's family", res.family, "the table's", family)
        own = own or res.batch
    return own


def decode_legs(sz, batches, codec, rows, R, nchunks, legs, tag, cs=None, **kw):
    """every leg on every container: the input, every return value, nothing outside, the family"""
    nrows, D = rows.shape
    cs = nchunks * R if cs is None else cs
    for no_fast, cpg, family in legs:
        for who, batch in batches:
            res = cr.decode(sz, batch, codec, rows.dtype.itemsize, D, R, cs, no_fast=no_fast, cpg=cpg, **kw)
            cr.check_decode(res, rows, tag + (family, cpg, who))
            assert res.family == family, (tag, "the planner's family", res.family, "the table's", family)


def both_containers(sz, oracle, codec, rows, R, own):
    D = rows.shape[1]
    return [("own container", own), ("the oracle's container", oracle_batch(sz, oracle, codec, D, rows.reshape(-1), R * D))]


# ------------------------------------------------------------------ 1. the run drive

@pytest.mark.parametrize("kind", rd.KINDS)
@pytest.mark.parametrize("codec", cr.BOTH)
@pytest.mark.parametrize("w,D", list(cr.RLE_SHAPES), ids=[f"u{w}x{D}" for w, D in cr.RLE_SHAPES])
def test_runs_through_every_edge(sz, oracle, w, D, codec, kind):
    """run lengths 1 .. 16 and 126 .. 129 closing in either slot, a run as the first slot, chunks ending in a run: a step that stages one
    packed block and then enters a run, and a leftover flush that depends on the steps that staged something"""
    _, encs, decs = cr.RLE_SHAPES[(w, D)]
    data, chunk_len, _ = batch_of(codec, w, D, kind, cr.RLE_NCHUNKS, cr.RLE_NB)
    rows, R = data.reshape(-1, D), chunk_len // D
    tag = ("runs", w, D, codec, kind)
    own = encode_legs(sz, oracle, codec, rows, R, encs, tag)
    decode_legs(sz, both_containers(sz, oracle, codec, rows, R, own), codec, rows, R, cr.RLE_NCHUNKS, decs, tag)


# ------------------------------------------------------------------ 2. the FIRE drive

@pytest.mark.parametrize("w,D", list(cr.FIRE_LEGS), ids=[f"u{w}x{D}" for w, D in cr.FIRE_LEGS])
def test_fire_counters_through_their_wrap(sz, oracle, w, D):
    """the int16 counter wrap and runs at frozen extreme coefficients, from a column-major source into a column-major destination"""
    nchunks = FIRE_SHAPES[(w, D)][0]
    data, chunk_len = fire_batch_of(w, D, nchunks)
    rows, R = data.reshape(-1, D), chunk_len // D
    encs, decs = cr.FIRE_LEGS[(w, D)]
    tag = ("fire", w, D)
    own = encode_legs(sz, oracle, "xff", rows, R, encs, tag)
    decode_legs(sz, both_containers(sz, oracle, "xff", rows, R, own), "xff", rows, R, nchunks, decs, tag)


# ------------------------------------------------------------------ 3. every lane mapping

@pytest.mark.parametrize("esz", (1, 2))
@pytest.mark.parametrize("D", list(cr.MAPPINGS))
def test_every_lane_mapping(sz, oracle, D, esz):
    """one, two and four columns a lane, every lane count, full and partly filled: 7 chunks, a ragged last one, a flat span across a seam"""
    dp, cpl = cr.MAPPINGS[D]
    codec = cr.BOTH[(list(cr.MAPPINGS).index(D) + esz) % 2]
    R, n = cr.MAP_ROWS, cr.MAP_NCHUNKS
    nrows = (n - 1) * R + cr.MAP_LAST
    rows = cr.walk(100 * D + esz, nrows, D, esz, R)
    tag = ("mapping", esz, D, codec)
    batch = oracle_batch(sz, oracle, codec, D, rows.reshape(-1), R * D)
    for cpg in (1, 3):
        res = cr.decode(sz, batch, codec, esz, D, R, n * R + 8, cpg=cpg)
        cr.check_decode(res, rows, tag + (cpg,))
        assert (res.family, res.plan["dp"], res.plan["cpl"]) == ("dec_fast", dp, cpl), (tag, res.plan)
    if D <= cr.MAP_ENCODE_MAX:
        encode_legs(sz, oracle, codec, rows, R, cr.ENC_FAST_LEGS[:2], tag, cs=n * R + 8)


# ------------------------------------------------------------------ 4. step parity and short ends

PARITY_CASES = [(w, D, R, last) for (w, D), tab in cr.PARITY_ROWS.items() for R in tab for last in cr.parity_lasts(R)]


@pytest.mark.parametrize("w,D,R,last", PARITY_CASES, ids=[f"u{w}x{D}-R{R}-last{last}" for w, D, R, last in PARITY_CASES])
def test_step_parity_and_short_ends(sz, oracle, w, D, R, last):
    """an odd and an even number of stream groups a chunk, each with and without a block behind them, and a last chunk that is nothing but a
    tail, one block, one group, a group and a tail: the flush on every second step, the leftover flush, the reset at the seam"""
    n = cr.PARITY_NCHUNKS
    rows = cr.parity_data(w, D, R, last)
    for codec in cr.BOTH:
        tag = ("parity", w, D, R, last, codec)
        own = encode_legs(sz, oracle, codec, rows, R, cr.ENC_FAST_LEGS[:2], tag, cs=n * R)
        decode_legs(sz, both_containers(sz, oracle, codec, rows, R, own), codec, rows, R, n, cr.DEC_FAST_LEGS[:2], tag)


# ------------------------------------------------------------------ 5. stride and alignment

def test_columns_abut(sz, oracle):
    """col_stride == nrows, the matrix a tight [D, nrows] tensor: the next column starts where this one ends.  Once a multiple of 8 (the fast
    kernels), once not (the generic ones)"""
    for R, legs_e, legs_d in ((64, cr.ENC_FAST_LEGS, cr.DEC_FAST_LEGS), (50, cr.ENC_GENERIC_LEGS, cr.DEC_GENERIC_LEGS)):
        n = 3
        rows = cr.walk(R, n * R, 8, 2, R)
        assert (n * R % 8 == 0) == (R == 64)
        for codec in cr.BOTH:
            tag = ("abut", R, codec)
            own = encode_legs(sz, oracle, codec, rows, R, legs_e, tag, tight=True)
            decode_legs(sz, both_containers(sz, oracle, codec, rows, R, own), codec, rows, R, n, legs_d, tag, tight=True)


@pytest.mark.parametrize("esz,D", [(2, 8), (1, 16)])
def test_base_off_the_16_byte_grid(sz, oracle, esz, D):
    """an aligned stride under a base shifted by one element and by 8 bytes: the planner's answer (the generic kernels) ran, the bytes are the
    same -- for the source of an encode and the destination of a decode"""
    R, n = 64, 4
    rows = cr.walk(7 * D, (n - 1) * R + 40, D, esz, R)
    for shift in (0, 1, 8 // esz):
        want_e, want_d = (("enc_pair", "enc_fast"), "dec_fast") if shift == 0 else (("enc_generic", "enc_generic"), "dec_generic")
        for codec in cr.BOTH:
            tag = ("shift", esz, D, shift, codec)
            own = encode_legs(sz, oracle, codec, rows, R, [(1, 0, want_e[0]), (0, 0, want_e[1])], tag, cs=n * R + 8, shift=shift)
            decode_legs(sz, both_containers(sz, oracle, codec, rows, R, own), codec, rows, R, n, [(0, 1, want_d), (0, 3, want_d)], tag,
                        cs=n * R + 8, shift=shift)


def test_stride_of_the_chunks_exactly(sz, oracle):
    """col_stride == nchunks x R -- the ragged last chunk's missing rows are all that separates two columns -- and eight more"""
    R, n, D = 72, 5, 8
    rows = cr.walk(11, (n - 1) * R + 19, D, 2, R)
    for cs in (n * R, n * R + 8):
        for codec in cr.BOTH:
            tag = ("stride", cs, codec)
            own = encode_legs(sz, oracle, codec, rows, R, cr.ENC_FAST_LEGS, tag, cs=cs)
            decode_legs(sz, both_containers(sz, oracle, codec, rows, R, own), codec, rows, R, n, cr.DEC_FAST_LEGS, tag, cs=cs)


# ------------------------------------------------------------------ 6. damage

@pytest.mark.parametrize("cpg", (1, 3))
@pytest.mark.parametrize("w,D,no_fast", list(cr.DAMAGE_SHAPES), ids=[f"u{w}x{D}-{f}" for (w, D, _), f in cr.DAMAGE_SHAPES.items()])
def test_damaged_chunk_stays_inside_its_rows(sz, oracle, w, D, no_fast, cpg):
    """a stream 5 bytes short and a header with another ndims, in the middle of a lane group of three: rets are decompress_batch's, negative for
    the damaged chunk; every other chunk's rows are exact; in every column nothing outside rows [c R, (c + 1) R) differs; guards and padding
    are intact"""
    import torch
    esz, R, n, bad = w // 8, cr.DAMAGE_ROWS, cr.DAMAGE_NCHUNKS, cr.DAMAGE_BAD
    family = cr.DAMAGE_SHAPES[(w, D, no_fast)]
    rows = cr.walk(13 * D + w, (n - 1) * R + 33, D, esz, R)
    for codec in cr.BOTH:
        good = oracle_batch(sz, oracle, codec, D, rows.reshape(-1), R * D)
        cd = sz.ChunkedCodec(codec, esz, D, R * D, device="cuda:0")
        for what, batch in (("5 bytes short", truncated_batch(sz, good, bad)), ("wrong ndims", cr.wrong_ndims(good, bad, D))):
            tag = ("damage", w, D, codec, what, cpg)
            res = cr.decode(sz, batch, codec, esz, D, R, n * R + 8, no_fast=no_fast, cpg=cpg)
            cr.check_decode(res, rows, tag, bad=(bad,))
            assert res.family == family, (tag, res.family)
            flat = torch.zeros(n * R * D, dtype=torch.int8 if esz == 1 else torch.int16, device="cuda").view(cd.dtype)
            rets = torch.full((n,), cr.RETS_SENT, dtype=torch.int64, device="cuda")
            with cr.knobs(no_fast=no_fast, cpg=cpg):
                cd.decompress_into(batch.data, batch.offsets, n, flat, rets)
            torch.cuda.synchronize()
            assert np.array_equal(res.rets[:n], rets.cpu().numpy()) and res.rets[bad] < 0, (tag, res.rets.tolist(), rets.cpu().numpy().tolist())


# ------------------------------------------------------------------ 7. reach

def need_memory(nbytes):
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (2 << 30):
        pytest.skip(f"{free >> 20} MiB of device memory free, the buffer takes {nbytes >> 20} MiB and 2 GiB more")


@pytest.mark.parametrize("which", ("cs_fast", "cs_generic"))
def test_decode_reach(sz, oracle, which):
    """the largest stride within reach of decode_fast.h's 32-bit offsets, D cs esz < 0xf0000000, and the next multiple of 8, which the generic
    kernel takes at 64-bit addresses: a destination of 4.03 GB, of which the rows written and 64 elements on either side of them in every
    column are filled with the sentinel and checked"""
    import torch
    k = cr.REACH_DEC
    esz, D, R, n, cs = k["esz"], k["D"], k["R"], k["nchunks"], k[which]
    family = {"cs_fast": "dec_fast", "cs_generic": "dec_generic"}[which]
    G = 64
    total = G + D * cs + G
    need_memory(total * esz)
    nrows = n * R - 3
    rows = cr.walk(5, nrows, D, esz, R)
    batch = oracle_batch(sz, oracle, "xff", D, rows.reshape(-1), R * D)
    out = torch.empty(total, dtype=torch.int16, device="cuda")
    s16 = int(np.array(cr.sent(esz), np.uint16).view(np.int16))
    for d in range(D):
        out[d * cs:d * cs + G + n * R + G] = s16         # (from 64 elements in front of the column's first row on: the buffer starts G in front of the matrix)
    rets = torch.full((n + 1,), cr.RETS_SENT, dtype=torch.int64, device="cuda")
    dst = out.data_ptr() + G * esz
    torch.cuda.synchronize()
    with cr.knobs():
        before = cr.counts()
        sz._lib.check(sz._lib.decompress_batch_colmajor(cr.CODEC_ID["xff"], esz, batch.data.data_ptr(), batch.offsets.data_ptr(), n, R, D, cs, dst,
                                                        rets.data_ptr(), None))
        ran = cr.moved(before, cr.counts())
    torch.cuda.synchronize()
    for d in range(D):
        got = out[d * cs:d * cs + G + n * R + G].cpu().numpy().view(np.uint16)
        want = np.full(got.size, cr.sent(esz), np.uint16)
        want[G:G + nrows] = rows[:, d]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (which, "column", d, "first wrong element at row", int(bad[0]) - G, int(got[bad[0]]), int(want[bad[0]]))
    r = rets.cpu().numpy()
    assert r[:n].tolist() == [min(R, nrows - c * R) * D for c in range(n)] and r[n] == cr.RETS_SENT, r
    assert cr.decode_plan("xff", esz, D, R, n, cs, 0, 1, dst & 15)["family"] == family
    cr.check_dispatch(ran, {family: 1}, only=[family], what=which)
    del out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("pair", (1, 0))
def test_encode_reach(sz, oracle, pair):
    """a column stride of 2^32 + 64 elements: encode_fast.h and encode_wide.h keep the stride of their burst loads in 32 bits, so the planner
    sends such a source to the generic kernel, whose stride is 64 bits wide.  Column d holds the walk offset by 37 d, so that a column read
    from another place gives other bytes.  17.2 GB from torch.empty, of which only the rows used are written"""
    import torch
    k = cr.REACH_ENC
    esz, D, R, n, cs = k["esz"], k["D"], k["R"], k["nchunks"], k["cs"]
    nrows = n * R
    total = (D - 1) * cs + nrows + sz._lib.READ_SLACK
    need_memory(total)
    base = cr.walk(3, nrows, 1, esz, R)[:, 0].astype(np.int64)
    rows = ((base[:, None] + 37 * np.arange(D)[None, :]) % 256).astype(DTYPES[esz])
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    for d in range(D):
        src[d * cs:d * cs + nrows] = torch.from_numpy(rows[:, d].copy()).cuda()
    ss = int(sz._lib.compress_bound(esz, R * D, D))
    slots = torch.full(((n + 1) * ss,), cr.BYTE, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n + 1,), cr.RETS_SENT, dtype=torch.int32, device="cuda")
    rets = torch.full((n + 1,), cr.RETS_SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with cr.knobs(pair=pair):
        before = cr.counts()
        sz._lib.check(sz._lib.compress_batch_colmajor(cr.CODEC_ID["xff"], esz, src.data_ptr(), nrows, cs, R, D, slots.data_ptr(), ss, sizes.data_ptr(),
                                                      rets.data_ptr(), None))
        ran = cr.moved(before, cr.counts())
    torch.cuda.synchronize()
    want, wrets = cr.expected(oracle, "xff", rows, R)
    s, z, r = slots.cpu().numpy(), sizes.cpu().numpy(), rets.cpu().numpy()
    for c, w in enumerate(want):
        assert z[c] == w.size and np.array_equal(s[c * ss:c * ss + w.size], w), ("chunk", c, "differs from the oracle's stream", ran)
        assert r[c] == wrets[c], (c, r, wrets)
    assert z[n] == cr.RETS_SENT and r[n] == cr.RETS_SENT and (s[n * ss:] == cr.BYTE).all()
    assert cr.encode_plan("xff", esz, D, R, nrows, cs, pair, 0, src.data_ptr() & 15)["family"] == "enc_generic"
    cr.check_dispatch(ran, {"enc_generic": 1}, only=["enc_generic"], what="encode reach")
    del src
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ 8. small things

def test_side_stream_twice_into_the_same_buffers(sz, oracle):
    import torch
    R, n, D = 64, 5, 8
    rows = cr.walk(21, (n - 1) * R + 17, D, 2, R)
    st = torch.cuda.Stream()
    for codec in cr.BOTH:
        enc = dec = None
        for turn in (0, 1):
            enc = cr.encode(sz, rows, codec, R, cs=n * R, stream=st, bufs=enc and enc.bufs)
            cr.check_encode(enc, oracle, codec, rows, ("side stream", codec, turn))
            dec = cr.decode(sz, enc.batch, codec, 2, D, R, n * R, cpg=3, stream=st, bufs=dec and dec.bufs)
            cr.check_decode(dec, rows, ("side stream", codec, turn))
        assert (enc.family, dec.family) == ("enc_pair", "dec_fast")


def test_empty_calls_launch_nothing_and_write_nothing(sz, oracle):
    """nrows == 0 on both encode entry points (the dense one sets the container's first offset, as its row-major form does) and nchunks == 0"""
    rows = np.zeros((0, 8), np.uint16)
    for dense in (False, True):
        res = cr.encode(sz, rows, "xff", 64, cs=64, dense=dense)
        if dense:
            assert res.offsets[0] == 0
        cr.check_encode(res, oracle, "xff", rows, ("empty", dense))
        assert not res.ran
    some = cr.walk(2, 128, 8, 2, 64)
    batch = oracle_batch(sz, oracle, "xff", 8, some.reshape(-1), 64 * 8)
    res = cr.decode(sz, batch, "xff", 2, 8, 64, 128, nchunks=0)
    cr.check_decode(res, rows, ("empty decode",))
    assert not res.ran


@pytest.mark.parametrize("esz,D", [(2, 8), (1, 32), (2, 100)])
def test_both_encode_entry_points_give_the_same_streams(sz, oracle, esz, D):
    R, n = 72, 6
    rows = cr.walk(17 * D, (n - 1) * R + 50, D, esz, R)
    for codec in cr.BOTH:
        a = cr.encode(sz, rows, codec, R, cs=n * R, dense=False)
        b = cr.encode(sz, rows, codec, R, cs=n * R, dense=True)
        for res in (a, b):
            cr.check_encode(res, oracle, codec, rows, ("entry points", esz, D, codec, res.dense))
        assert a.family == b.family == ("enc_pair" if D <= 64 else "enc_generic")
        assert np.array_equal(a.sizes, b.sizes) and np.array_equal(a.rets, b.rets)
        assert all(np.array_equal(a.slots[c * a.ss:c * a.ss + a.sizes[c]], b.slots[c * b.ss:c * b.ss + b.sizes[c]]) for c in range(n))
