"""CPU tests of the planner (sprintz_amd/csrc/plan.h): which kernel family serves a call is plain integer arithmetic on a shape, the
dispatch options and a few address low bits, so the edges the GPU tier pins with the dispatch counters are checked here without a
device.  tests/plan_probe.cpp includes plan.h, is built with g++ -- which is itself the check that plan.h and geom.h hold no HIP -- and
answers one query per line.

1. the GPU edge table (tests/dispatch_cases.py), replayed: decode family, encode family, and how the container is built;
2. the other pinned edges with today's literals: gather rows, write_size, the 4 GB output edge of decode_row.h;
3. properties read off the code, over a sweep of esz 1 / 2, every ndims in 1 .. 512 plus 513, 2047, 2048 and 65 535, five chunk lengths
   (15 / 16 / 128 rows-of-ndims, 5 120 and 10 240 elements rounded up to rows), six batch sizes and both RLE codecs on default options:
   exactly one of plan and error, the same answer twice; with no_fast every shape of at most 512 columns on the generic kernels; a
   host-call input is dec_lat / enc_lat exactly when the same single chunk is without the flag (what the ticket path relies on);
   dec_fast's lane group holds the columns and is more than half full; dynamic LDS at most 160 KB and a grid in 1 .. 2^31 - 1."""
import pytest

import planner
from dispatch_cases import CASES, ENC, GATHER_EDGES, OPTION_DEFAULTS
from planner import CODEC, bound, probe  # noqa: F401  (fixtures)



def knobs(lat=OPTION_DEFAULTS["lat"], blk_chunks=OPTION_DEFAULTS["blk_chunks"], mask=OPTION_DEFAULTS["mask"], pair=OPTION_DEFAULTS["pair"]):
    return dict(lat_chunks=lat, blk_chunks=blk_chunks, blk_kernels=mask, enc_pair=pair)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_gpu_edge_table_replayed(probe, case):
    tag, opts, codec, esz, D, chunk_len, nchunks, enc, dec, kw = case
    assert set(kw) <= {"align", "src_shift", "out_shift", "comp_shift"}
    shape = dict(codec=CODEC[codec], esz=esz, D=D, chunk_len=chunk_len, nchunks=nchunks, total_len=nchunks * chunk_len, slot_stride=bound(esz, chunk_len, D), **knobs(**opts))
    if dec:
        got, = probe(("decode", dict(shape, out_lo=kw.get("out_shift", 0) * esz % 16, comp_lo=kw.get("comp_shift", 0) % 16)))
        assert got.get("family") == dec, (tag, got)
    if enc:
        want_enc = [k for k in enc if k.startswith("enc_")]
        want_dense, = [k for k in enc if k.startswith("dense_")]
        if kw.get("src_shift") or kw.get("align", 16) != 16:        # the slot path followed by compact
            got, = probe(("encode", dict(shape, src_lo=kw.get("src_shift", 0) % 16)))
            assert [got.get("family")] == want_enc and got.get("fused") == 0 and want_dense == "dense_compact", (tag, got)
        else:                                                       # ChunkedCodec.compress: compress_batch_dense
            got, = probe(("dense", shape))
            assert got.get("family") == want_dense and [got.get("enc")] == (want_enc or ["none"]), (tag, got)


@pytest.mark.parametrize("esz,D,out_shift,family", GATHER_EDGES)
def test_gather_rows_edges(probe, esz, D, out_shift, family):
    R, nchunks, rows = 64, 9, 70
    got, = probe(("gather", dict(codec=CODEC["xff"], esz=esz, D=D, chunk_len=R * D, nchunks=nchunks, nranges=6, rows=rows, out_lo=out_shift * esz % 16)))
    assert got.get("family") == family, got


@pytest.mark.parametrize("write_size,family", [(True, "enc_blk"), (False, "enc_pair")])
def test_encode_blk_writes_the_stream_header_itself(probe, write_size, family):
    """a single call of 2 048 uint8 x 16: one chunk, planned first as a host call for the staging addresses, then for the staged source"""
    D, n = 16, 2048
    shape = dict(codec=CODEC["delta"], esz=1, D=D, chunk_len=n, nchunks=1, total_len=n, slot_stride=bound(1, n, D), write_size=write_size, **knobs(**ENC))
    ticket, staged = probe(("encode", dict(shape, host_call=1)), ("encode", shape))
    assert ticket.get("family") != "enc_lat" and staged.get("family") == family, (ticket, staged)


def test_an_output_of_4_GB_stays_on_the_older_kernel(probe):
    """decode_row.h addresses its output with 32-bit offsets: 0xf0000000 bytes or more are the lane-per-column kernel's, one chunk less
    is decode_row.h's (the GPU tier needs 4 GB of HBM twice for this)"""
    D, chunk_len = 32, 32768
    nchunks = 0xf0000000 // chunk_len
    shape = dict(codec=CODEC["delta"], esz=1, D=D, chunk_len=chunk_len, **knobs(lat=0, blk_chunks=1, mask=9))
    at, below = probe(("decode", dict(shape, nchunks=nchunks)), ("decode", dict(shape, nchunks=nchunks - 1)))
    assert at.get("family") == "dec_fast" and below.get("family") == "dec_row", (at, below)


@pytest.mark.parametrize("pair,family", [(1, "enc_pair"), (0, "enc_fast")])
def test_a_column_stride_of_2_to_the_32_stays_on_the_generic_encoder(probe, pair, family):
    """encode_fast.h and encode_wide.h keep a column-major source's stride as a 32-bit element count in their burst loads: 2^32 elements or
    more are the generic kernel's (a 64-bit stride), eight less is theirs (the GPU tier needs 17 GB of HBM for this)"""
    D, R, nchunks = 8, 64, 3
    shape = dict(codec=CODEC["xff"], esz=2, D=D, chunk_len=R * D, nchunks=nchunks, total_len=nchunks * R * D, slot_stride=bound(2, R * D, D), **knobs(pair=pair))
    at, below = probe(("encode", dict(shape, col_stride=1 << 32)), ("encode", dict(shape, col_stride=(1 << 32) - 8)))
    assert at.get("family") == "enc_generic" and below.get("family") == family, (at, below)


# shapes on which the PARENT's logic already violates a property of the sweep: findings, not behaviour changes (at most 1 % of the sweep)
SWEEP_KNOWN = ()


def test_properties_over_the_sweep(probe):
    out = planner.run("sweep\n")
    shapes = int(out[-1].split("shapes=")[1].split()[0])
    assert shapes == 2 * 516 * 5 * 6 * 2
    violations = [line for line in out[:-1] if not any(known in line for known in SWEEP_KNOWN)]
    assert len(out) - 1 - len(violations) <= shapes // 100
    assert not violations, (len(violations), violations[:20])


def test_the_mode_numbers_are_geom_hs(probe):
    """planner.QUERY, the one table of mode numbers the tests use, against the kQuery* constants themselves"""
    assert {name.lower().replace("_", ""): v for name, v in planner.QUERY.items()} == {name.lower(): v for name, v in planner.modes().items()}
