"""CPU tier of the column-major drive (tests/test_gpu_colmajor.py, tests/test_gpu_colmajor_drive.py), without a device: every kernel family the
GPU tier names is what csrc/plan.h plans for that call on a host compiler; the smallest row counts it uses are the planner's own boundaries; the
reach boundaries of both sides are where the GPU tier puts its two large buffers; and the chunks of the step-parity test have the stream groups
and tails it claims, counted in the oracle's streams."""
import numpy as np

import colmajor_runner as cr
import rle_drive as rd
from drive_tables import FIRE_SHAPES
from planner import probe  # noqa: F401  (a fixture: skips without g++)
from streams import fire_batch_of


def enc(codec, esz, D, R, nrows, cs, pair=1, no_fast=0, src_lo=0):
    return cr.encode_plan(codec, esz, D, R, nrows, cs, pair, no_fast, src_lo).get("family")


def dec(codec, esz, D, R, nchunks, cs, no_fast=0, cpg=1, out_lo=0):
    return cr.decode_plan(codec, esz, D, R, nchunks, cs, no_fast, cpg, out_lo).get("family")


def test_the_twelve_shapes_literals_are_the_planners(probe):
    for name, codec, esz, D, R, nrows, cs, enc_two, enc_one, want in cr.CM_CONFIGS:
        cs = cs or nrows
        n = cr.chunks_of(nrows, R)
        assert (enc(codec, esz, D, R, nrows, cs, 1), enc(codec, esz, D, R, nrows, cs, 0)) == (enc_two, enc_one), name
        assert dec(codec, esz, D, R, n, n * R + 8) == want, name          # (the test's destination: [D, nchunks x R + 8])


def test_the_drives_literals_are_the_planners(probe):
    """the run drive's and the FIRE drive's legs, both codecs"""
    shapes = [(w, D, cr.RLE_NCHUNKS, 8 * cr.RLE_NB, e, d) for (w, D), (_, e, d) in cr.RLE_SHAPES.items()]
    shapes += [(w, D, FIRE_SHAPES[(w, D)][0], fire_batch_of(w, D, FIRE_SHAPES[(w, D)][0])[1] // D, e, d) for (w, D), (e, d) in cr.FIRE_LEGS.items()]
    for w, D, n, R, encs, decs in shapes:
        for codec in cr.BOTH:
            for pair, no_fast, family in encs:
                assert enc(codec, w // 8, D, R, n * R, n * R, pair, no_fast) == family, (w, D, codec, pair, no_fast)
            for no_fast, cpg, family in decs:
                assert dec(codec, w // 8, D, R, n, n * R, no_fast, cpg) == family, (w, D, codec, no_fast, cpg)


def test_every_lane_mapping_is_the_planners(probe):
    """dec_fast with the lanes a chunk and the columns a lane the table claims, at MAP_ROWS rows a chunk on both widths; both fast encoders up to
    64 columns, none above"""
    R, n = cr.MAP_ROWS, cr.MAP_NCHUNKS
    nrows, cs = (n - 1) * R + cr.MAP_LAST, n * R + 8
    for esz in (1, 2):
        assert R >= max(cr.min_fast_rows(esz, D) for D in cr.MAPPINGS)
        for D, (dp, cpl) in cr.MAPPINGS.items():
            for codec in cr.BOTH:
                for cpg in (1, 3):
                    p = cr.decode_plan(codec, esz, D, R, n, cs, 0, cpg)
                    assert (p.get("family"), p.get("dp"), p.get("cpl"), p.get("chunks_per_group")) == ("dec_fast", dp, cpl, cpg), (esz, D, codec, p)
                want = ("enc_pair", "enc_fast") if D <= cr.MAP_ENCODE_MAX else ("enc_generic", "enc_generic")
                assert (enc(codec, esz, D, R, nrows, cs, 1), enc(codec, esz, D, R, nrows, cs, 0)) == want, (esz, D, codec)


def test_the_smallest_row_counts_are_the_planners_boundary(probe):
    """taken at R, not at R - 8: the step-parity test's first row count on either shape, and the decode reach test's"""
    for (w, D), tab in cr.PARITY_ROWS.items():
        first = min(tab)
        assert cr.min_fast_rows(w // 8, D) == first, (w, D)
        for codec in cr.BOTH:
            assert dec(codec, w // 8, D, first, cr.PARITY_NCHUNKS, cr.PARITY_NCHUNKS * first) == "dec_fast"
            assert dec(codec, w // 8, D, first - 8, cr.PARITY_NCHUNKS, cr.PARITY_NCHUNKS * (first - 8)) == "dec_generic"
    k = cr.REACH_DEC
    assert cr.min_fast_rows(k["esz"], k["D"]) == k["R"]


def test_parity_legs_and_strides_are_the_planners(probe):
    """the step-parity test's legs at every row count and short end; columns that abut; a base off the 16-byte grid; the exact stride; damage"""
    for (w, D), tab in cr.PARITY_ROWS.items():
        for R in tab:
            for last in cr.parity_lasts(R):
                n = cr.PARITY_NCHUNKS
                nrows = (n - 1) * R + last
                for codec in cr.BOTH:
                    assert (enc(codec, w // 8, D, R, nrows, n * R, 1), enc(codec, w // 8, D, R, nrows, n * R, 0)) == ("enc_pair", "enc_fast"), (w, D, R, last)
                    assert {dec(codec, w // 8, D, R, n, n * R, 0, cpg) for cpg in (1, 3)} == {"dec_fast"}, (w, D, R, last)
    for codec in cr.BOTH:
        # columns that abut: a stride of whole blocks, and one that is not
        for R, encs, decs in ((64, cr.ENC_FAST_LEGS, cr.DEC_FAST_LEGS), (50, cr.ENC_GENERIC_LEGS, cr.DEC_GENERIC_LEGS)):
            for pair, no_fast, family in encs:
                assert enc(codec, 2, 8, R, 3 * R, 3 * R, pair, no_fast) == family, (R, pair, no_fast)
            for no_fast, cpg, family in decs:
                assert dec(codec, 2, 8, R, 3, 3 * R, no_fast, cpg) == family, (R, no_fast, cpg)
        # a base one element and 8 bytes off the grid, under an aligned stride
        for esz, D in ((2, 8), (1, 16)):
            nrows, cs = 3 * 64 + 40, 4 * 64 + 8
            for lo in (esz, 8):
                assert (enc(codec, esz, D, 64, nrows, cs, 1, 0, lo), enc(codec, esz, D, 64, nrows, cs, 0, 0, lo)) == ("enc_generic", "enc_generic")
                assert dec(codec, esz, D, 64, 4, cs, 0, 3, lo) == "dec_generic"
            assert (enc(codec, esz, D, 64, nrows, cs, 1), enc(codec, esz, D, 64, nrows, cs, 0), dec(codec, esz, D, 64, 4, cs)) == ("enc_pair", "enc_fast", "dec_fast")
        # a stride of the chunks exactly, and eight more
        for cs in (5 * 72, 5 * 72 + 8):
            for pair, no_fast, family in cr.ENC_FAST_LEGS:
                assert enc(codec, 2, 8, 72, 4 * 72 + 19, cs, pair, no_fast) == family
            for no_fast, cpg, family in cr.DEC_FAST_LEGS:
                assert dec(codec, 2, 8, 72, 5, cs, no_fast, cpg) == family
        for (w, D, no_fast), family in cr.DAMAGE_SHAPES.items():
            for cpg in (1, 3):
                assert dec(codec, w // 8, D, cr.DAMAGE_ROWS, cr.DAMAGE_NCHUNKS, cr.DAMAGE_NCHUNKS * cr.DAMAGE_ROWS + 8, no_fast, cpg) == family, (w, D, no_fast)
        # the small things
        assert (enc(codec, 2, 8, 64, 4 * 64 + 17, 5 * 64), dec(codec, 2, 8, 64, 5, 5 * 64, 0, 3)) == ("enc_pair", "dec_fast")
        for esz, D in ((2, 8), (1, 32), (2, 100)):
            assert enc(codec, esz, D, 72, 5 * 72 + 50, 6 * 72) == ("enc_pair" if D <= 64 else "enc_generic")


def test_the_reach_boundaries(probe):
    """decode: decode_fast.h below D cs esz = 0xf0000000, the generic kernel from there on.  Encode: the fast kernels up to a stride of
    2^32 - 8 elements, the generic kernel from 2^32 on -- their burst loads keep the stride in 32 bits"""
    k = cr.REACH_DEC
    esz, D, R, n = k["esz"], k["D"], k["R"], k["nchunks"]
    assert k["cs_fast"] % 8 == 0 and k["cs_generic"] == k["cs_fast"] + 8
    assert D * k["cs_fast"] * esz < 0xf0000000 <= D * k["cs_generic"] * esz
    for codec in cr.BOTH:
        for cpg in (1, 3):
            assert dec(codec, esz, D, R, n, k["cs_fast"], 0, cpg) == "dec_fast" and dec(codec, esz, D, R, n, k["cs_generic"], 0, cpg) == "dec_generic"
    k = cr.REACH_ENC
    esz, D, R, n = k["esz"], k["D"], k["R"], k["nchunks"]
    assert k["cs"] % 8 == 0 and k["cs"] >= 1 << 32
    for codec in cr.BOTH:
        for e2, D2 in ((esz, D), (2, 8), (1, 64)):
            for pair, want in ((1, "enc_pair"), (0, "enc_fast")):
                assert enc(codec, e2, D2, R, n * R, (1 << 32) - 8, pair) == want, (codec, e2, D2, pair)
                for cs in (1 << 32, k["cs"], 1 << 40):
                    assert enc(codec, e2, D2, R, n * R, cs, pair) == "enc_generic", (codec, e2, D2, pair, cs)


def test_parity_chunks_have_the_groups_and_tails_claimed(oracle):
    """counted in the stream the oracle writes: a full chunk's stream groups and the rows of its verbatim tail, and the last chunk's"""
    seen = set()
    for (w, D), tab in cr.PARITY_ROWS.items():
        for R, full in tab.items():
            for last, short in cr.parity_lasts(R).items():
                rows = cr.parity_data(w, D, R, last)
                assert rows.shape == ((cr.PARITY_NCHUNKS - 1) * R + last, D)
                for codec in cr.BOTH:
                    streams, _ = cr.expected(oracle, codec, rows, R)
                    got = [rd.slots(s, w, D)[:2] for s in streams]
                    assert all(sl[2] == "block" for s in streams for sl in rd.slots(s, w, D)[2]), (w, D, R, last, codec, "a run or a padding slot")
                    assert [(g, rem // D) for g, rem in got] == [full] * (cr.PARITY_NCHUNKS - 1) + [short], (w, D, R, last, codec, got)
                seen.add((full[0] % 2, full[1]))
        assert seen == {(1, 0), (1, 8), (0, 0), (0, 8)}, (w, D, seen)
        seen.clear()


def test_the_walks_flat_span_crosses_a_seam():
    """the mapping test's data: constant rows on both sides of the seam between chunks 1 and 2"""
    R = cr.MAP_ROWS
    x = cr.walk(1, 7 * R, 5, 2, R).astype(np.int64)
    flat = np.flatnonzero((np.diff(x, axis=0) == 0).all(axis=1))
    assert flat.min() < 2 * R - 16 and flat.max() >= 2 * R + 16
