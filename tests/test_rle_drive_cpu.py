"""CPU tier of the run drive: tests/rle_drive.py steers the RLE / group state machine through its edges.  Here, without a
device: the oracle's streams of those inputs parse to exactly the slots an independent restatement of A.5 predicts, the oracle inverts them,
the batches COVER the edges (asserted on the parsed slots, so a schedule that stops reaching an edge fails here and not silently), the
`<=` / `<` tail rule shows where it must and nowhere else, and the oracle's streams are the compiled reference's
(tests/golden/golden_rledrive_v1, minted by oracle/gen_golden_rledrive.py; tests/test_oracle_vs_ref.py where the reference is built).
The GPU tier (tests/test_gpu_rle_drive.py) runs every kernel family on the same inputs."""
import json
import os
import zlib

import numpy as np
import pytest

import rle_drive as rd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_rledrive_v1")
NCHUNKS, NBLOCKS = 16, 256
SHAPES = [(8, 1), (8, 5), (8, 8), (16, 2), (16, 8)]            # a low-dim and a general layout per width; 8 x 5: rows that end inside a byte


def tail_le(codec, w, D):
    return codec == "xff" and not rd.is_lowdim(w, D)


def parsed(oracle, codec, w, D, kind, r=0, nchunks=NCHUNKS, nblocks=NBLOCKS):
    """-> per chunk (ngroups, remaining_len, slots) of the oracle's stream, checked against the model and decoded back"""
    x, chunk_len, zero = rd.batch(codec, w, D, kind, nchunks, nblocks, r)
    out = []
    for c, s in enumerate(oracle.compress_chunks(codec, x, chunk_len, D)):
        got = rd.slots(s, w, D)
        want = rd.model_slots(zero[c], chunk_len, D, 8, tail_le(codec, w, D))
        assert got[:2] == want[:2], (codec, w, D, kind, r, "chunk", c, "ngroups, remaining_len", got[:2], "model", want[:2])
        assert got[2] == want[2], (codec, w, D, kind, r, "chunk", c, "first differing slot", next((a, b) for a, b in zip(got[2], want[2]) if a != b))
        d, ret = oracle.decompress(codec, s, w // 8, chunk_len)
        assert ret == chunk_len and np.array_equal(d, x[c * chunk_len:(c + 1) * chunk_len]), (codec, w, D, kind, r, c)
        out.append(got)
    return out


@pytest.mark.parametrize("kind", rd.KINDS)
@pytest.mark.parametrize("w,D", SHAPES)
@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_oracle_streams_are_the_models_slots(oracle, codec, w, D, kind):
    """also at chunk lengths that are no whole blocks, and at the short chunks the widest kernels get (48 and 51 blocks)"""
    for r in (0, 1, 8 * D - 1):
        parsed(oracle, codec, w, D, kind, r)
    for nblocks in (48, 51):
        parsed(oracle, codec, w, D, kind, 0, nblocks=nblocks)


def test_schedules_rotate_every_edge():
    """over 16 chunks the first run edge of a schedule sits on 16 consecutive block indices, and the packed blocks in front of a run
    cycle through 1, 2, 3"""
    for kind in ("lengths", "varint", "alternate"):
        first = [int(np.argmax(rd.schedule(kind, NBLOCKS, c))) for c in range(16)]
        assert [f - first[0] for f in first] == list(range(16)), (kind, first)
    z = rd.schedule("lengths", NBLOCKS, 0)
    edges = np.flatnonzero(np.diff(z.astype(int)))                     # run starts (odd positions) and ends
    gaps = edges[2::2] - edges[1:-1:2]
    assert set(gaps[:6].tolist()) == {1, 2, 3}
    assert all(rd.schedule("start", NBLOCKS, c)[0] for c in range(16))
    assert not rd.schedule("start", NBLOCKS, 0)[1] and rd.schedule("start", NBLOCKS, 1)[1]
    alt = rd.schedule("alternate", NBLOCKS, 0)
    assert alt[0] and not alt[1] and alt[:128:2].all() and not alt[1:128:2].any() and not rd.schedule("alternate", NBLOCKS, 1)[0]


@pytest.mark.parametrize("w,D", SHAPES)
@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_the_drive_covers_the_edges(oracle, codec, w, D):
    """Every edge of A.5, on the slots parsed from the oracle's streams of the five batches.  (A group always fills both slots, so a
    stream never ends in a packed block in slot 0: "a packed block ends the stream, in each slot" is the packed block BEHIND the last
    run -- in slot 1 of the run's group, and in slot 0 of a new one -- and a last group of two packed blocks.  Under the `<` test a
    last group of [run, packed block] needs a chunk that is no whole blocks: behind the run's last block two whole blocks and more must
    remain, and behind the packed one less than two -- so the "tails" batch is taken at r = 1 as well.)"""
    streams = [s for kind in rd.KINDS for s in parsed(oracle, codec, w, D, kind)] + parsed(oracle, codec, w, D, "tails", r=1)
    runs = {(L, b) for _, _, sl in streams for _, b, k, L in sl if k == "run"}
    missing = [(L, b) for L in list(range(1, 17)) + [126, 127, 128, 129] for b in (0, 1) if (L, b) not in runs]
    assert not missing, ("run lengths that never close in a slot", missing)
    assert any(L <= 127 for L, _ in runs) and any(L > 127 for L, _ in runs)
    rolls = [(sl[j], sl[j + 1]) for _, _, sl in streams for j in range(len(sl) - 1) if sl[j][1:3] == (1, "run")]
    assert any(nxt[2] == "block" and nxt[:2] == (cur[0] + 1, 0) for cur, nxt in rolls), "no run in slot 1 followed by a packed block that opens a group"
    assert any(sl[0][2] == "run" and sl[0][3] == 1 for _, _, sl in streams) and any(sl[0][2] == "run" and sl[0][3] > 1 for _, _, sl in streams)
    ends = {tuple((b, k) for _, b, k, _ in sl[-2:]) for _, _, sl in streams}
    assert ((0, "run"), (1, "pad")) in ends, "no stream ends in a run in slot 0 and the padding slot"
    assert any(e[-1] == (1, "run") for e in ends), "no stream ends in a run in slot 1"
    assert ((0, "run"), (1, "block")) in ends, "no stream ends in [run, packed block]"
    assert ((0, "block"), (1, "block")) in ends, "no stream ends in two packed blocks"
    assert any(len(sl) >= 3 and sl[-3][1:3] == (1, "run") and [e[2] for e in sl[-2:]] == ["block", "block"] for _, _, sl in streams), \
        "no stream ends in a run in slot 1 and a packed block in slot 0 of a new group"
    assert sum(k == "pad" for _, _, sl in streams for _, _, k, _ in sl) == sum(sl[-1][2] == "pad" for _, _, sl in streams), "a padding slot inside a stream"


@pytest.mark.parametrize("w,D", [(8, 5), (8, 8), (16, 8)])
def test_the_tail_rule(oracle, w, D):
    """quirk 3 of SURVEY.md Appendix B: at chunk lengths of whole blocks that end in zero blocks, the general FIRE stream's last run takes
    one block more than the delta stream's (`<=` against `<` behind a run block); at r = 1 and r = 8 D - 1 more elements both take the same.
    The two tests differ where a run block leaves exactly two blocks: a chunk has to end in three zero blocks or more to get there; with
    one or two, both encoders stop at the same block (the "tails" batch ends in 1, 2, 3 and 5)"""
    be = 8 * D
    for r, more in ((0, 1), (1, 0), (be - 1, 0)):
        n = NBLOCKS * be + r
        used = {codec: [(n - rem) // be for _, rem, _ in parsed(oracle, codec, w, D, "tails", r)] for codec in ("delta", "xff")}
        zeros_at_end = {c: int(np.argmin(rd.schedule("tails", NBLOCKS, c)[::-1])) for c in range(NCHUNKS)}
        assert [zeros_at_end[c] for c in (0, 4, 8, 12)] == [1, 2, 3, 5]
        for c in (8, 12):
            assert used["xff"][c] == used["delta"][c] + more, (r, c, used["xff"][c], used["delta"][c])
            assert used["xff"][c] == NBLOCKS - 1 and used["delta"][c] == (NBLOCKS - 2 if r == 0 else NBLOCKS - 1), (r, c)
        for c in (0, 4):
            assert used["xff"][c] == used["delta"][c], (r, c, used["xff"][c], used["delta"][c])
    # the low-dim FIRE codec tests `<` like the delta codecs
    for wl, Dl in ((8, 1), (16, 2)):
        a, b = (parsed(oracle, codec, wl, Dl, "tails") for codec in ("delta", "xff"))
        assert [s[:2] for s in a] == [s[:2] for s in b] and [s[2] for s in a] == [s[2] for s in b]


@pytest.mark.parametrize("codec", ["delta", "xff"])
@pytest.mark.parametrize("w,D", [(8, 1), (8, 5)])
def test_the_cap(oracle, codec, w, D):
    """70 000 all-zero blocks and two packed ones: runs of 32 767, 32 767 and the rest, each closed by the cap into the next slot"""
    x, chunk_len, zero = rd.cap_chunks(codec, w, D, nchunks=1)
    s, _ = oracle.compress(codec, x, D)
    got = rd.slots(s, w, D)
    assert got == rd.model_slots(zero[0], chunk_len, D, 8, tail_le(codec, w, D))
    assert got[2][:3] == [(0, 0, "run", rd.CAP), (0, 1, "run", rd.CAP), (1, 0, "run", 70000 - 2 * rd.CAP)]
    # (`<` stops behind the last zero block, two blocks from the end: the padding slot; `<=` goes on to the first packed block)
    assert got[2][3:] == [(1, 1, "block", 1) if tail_le(codec, w, D) else (1, 1, "pad", 0)]


def test_samples_have_the_scheduled_zero_blocks():
    """the delta inputs by their own arithmetic: a block is all-zero exactly where the schedule says, the packed blocks mix widths in one
    row, and the batch builds fast enough to be rebuilt by every test"""
    import time
    for w, D in ((8, 5), (16, 8), (8, 80)):
        zero = rd.schedules("lengths", NCHUNKS, NBLOCKS)
        t0 = time.perf_counter()
        x = rd.samples("delta", w, D, zero, seed=3)
        assert time.perf_counter() - t0 < 1.0
        d = np.diff(np.concatenate([np.zeros((NCHUNKS, 1, D), np.int64), x.astype(np.int64)], axis=1), axis=1) & ((1 << w) - 1)
        assert np.array_equal(~d.reshape(NCHUNKS, NBLOCKS, 8 * D).any(axis=2), zero)
        zz = np.where(d >= 1 << (w - 1), (1 << w) - d, d)
        assert len(np.unique(zz.max(axis=1))) >= 5, "the columns' amplitudes do not differ"


def load_golden():
    with open(GOLDEN + ".json") as f:
        manifest = json.load(f)["cases"]
    return manifest, np.load(GOLDEN + ".npz")


def golden_input(m):
    """the fixture's input: chunk 0 of the batch its manifest entry names"""
    x, chunk_len, _ = rd.batch(m["codec"], m["w"], m["ndims"], m["kind"], m["nchunks"], m["nblocks"])
    return x[:chunk_len]


def test_golden_streams_are_the_oracles(oracle):
    """the fixture pins the generator (CRC32 of every input) and holds the oracle to the compiled reference's bytes"""
    manifest, arrays = load_golden()
    assert sorted({(m["codec"], m["w"], m["ndims"], m["kind"]) for m in manifest}) == sorted(
        (codec, w, D, kind) for codec in ("delta", "xff") for w, D in ((8, 1), (8, 8), (16, 2), (16, 8)) for kind in ("lengths", "varint", "tails"))
    for m in manifest:
        x = golden_input(m)
        assert x.size == m["n"] and zlib.crc32(x.tobytes()) == m["input_crc32"], (m, "the generator's output changed")
        got, ret = oracle.compress(m["codec"], x, m["ndims"])
        assert ret == m["ret"] and np.array_equal(got, arrays[m["name"]]), m


# ------------------------------------------------------------------ the GPU tier's kernel-family literals, replayed through the planner

from drive_tables import CAP_CASES, CASES, LAT_SINGLE, NB, NCHUNKS as ROWOP_NCHUNKS, ROWOP_SHAPES, family_of  # noqa: E402
from planner import QUERY, plan_shape, probe  # noqa: E402,F401  (probe: a fixture)
from streams import DEF, OLD  # noqa: E402

ROW_OPS = ("window", "filter", "select", "aggregate")


def test_the_gpu_tiers_literals_are_the_planners(probe):
    """every kernel family tests/test_gpu_rle_drive.py asserts from the dispatch counters is what csrc/plan.h plans for that shape and
    those options: a literal that is wrong fails here, without a device"""
    for tag, codecs, opts, w, D, nchunks, nblocks, r, enc, dec in CASES:
        for codec in codecs:
            shape = plan_shape(codec, w, D, 8 * nblocks * D + r, nchunks, **opts)
            dense, decode = probe(("dense", shape), ("decode", shape))
            assert dense.get("enc") == family_of(enc)[0] and decode.get("family") == family_of(dec)[0], (tag, codec, dense, decode)
    for w, D, nblocks, r in LAT_SINGLE:
        for codec in ("delta", "xff"):
            shape = plan_shape(codec, w, D, 8 * nblocks * D + r, 1, **DEF)
            dense, decode = probe(("dense", shape), ("decode", shape))
            assert dense.get("enc") == "enc_lat" and decode.get("family") == "dec_lat", (w, D, r, codec, dense, decode)
    for tag, opts, w, D, enc, dec in CAP_CASES:
        for codec in ("delta", "xff"):
            shape = plan_shape(codec, w, D, 8 * 70002 * D, 3, **opts)
            dense, decode = probe(("dense", shape), ("decode", shape))
            assert dense.get("enc") == enc and decode.get("family") == dec, (tag, codec, dense, decode)
    for (w, D), want in ROWOP_SHAPES.items():
        for codec in ("delta", "xff"):
            for no_fast in (0, 1):
                shape = plan_shape(codec, w, D, 8 * NB * D, ROWOP_NCHUNKS, no_fast=no_fast, **OLD)
                for op in ROW_OPS:
                    got, = probe(("decode", dict(shape, q=QUERY[op])))
                    assert got.get("family") == ("dec_generic" if no_fast else want[op]), (w, D, codec, op, no_fast, got)
                got, = probe(("gather", dict(shape, nranges=64, rows=11)))
                assert got.get("family") == ("gather_generic" if no_fast else want["gather"]), (w, D, codec, no_fast, got)
