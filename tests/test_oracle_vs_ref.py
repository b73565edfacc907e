"""CPU tests: oracle vs the compiled reference itself (oracle/_ref), over the
input families and sizes of the reference's own test-suite
(cpp/Compress/test/compress_testing.hpp:124-204,452-486).  Skipped when the
reference has not been built (it can only be built where /root/reference is)."""
import numpy as np
import pytest

from harness import (REF_TEST_SIZES, gen_fuzz, gen_patterns, gen_sparse, gen_walk)
from codec_helpers import oracle_pack, orc  # noqa: F401  (fixtures)


def _check(oracle, reference, codec, data, ndims):
    esz = data.dtype.itemsize
    so, ro = oracle.compress(codec, data, ndims)
    buf, rr = reference.compress_raw(codec, data, ndims)
    assert ro == rr
    assert np.array_equal(buf[:so.size], so)
    do, dro = oracle.decompress(codec, so, esz, data.size)
    assert dro == data.size and np.array_equal(do, data.ravel())
    dr, drr = reference.decompress(codec, so, esz, data.size, ndims)
    if not (drr == data.size and np.array_equal(dr, data.ravel())):
        # only legal divergence: the reference's 16-bit FIRE run replay
        assert codec == "xff" and esz == 2 and ndims >= 3
        dq, _ = oracle.decompress(codec, so, esz, data.size, quirk=1)
        assert np.array_equal(dq, dr)


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_families_match_reference(oracle, reference, codec, esz):
    rng = np.random.default_rng(123)
    for ndims in [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 33, 64, 65, 80, 129]:
        for n in REF_TEST_SIZES + [5120]:
            for _, d in gen_patterns(n, esz):
                _check(oracle, reference, codec, d, ndims)
            for sh in (0, 2, 4, 6, 9, 12, 14):
                if sh < 8 * esz:
                    _check(oracle, reference, codec, gen_fuzz(rng, n, esz, sh), ndims)
            _check(oracle, reference, codec, gen_sparse(rng, n, esz, 0.02), ndims)
            _check(oracle, reference, codec, gen_walk(rng, n, ndims, esz, 8), ndims)
            _check(oracle, reference, codec, gen_walk(rng, n, ndims, esz, 30, flat_every=3), ndims)


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_write_size_false_matches_reference(oracle, reference, codec, esz):
    rng = np.random.default_rng(5)
    for ndims in (1, 3, 8, 17):
        for n in (100, 16 * ndims * 5 + 3):
            d = gen_walk(rng, n, ndims, esz, 8)
            so, ro = oracle.compress(codec, d, ndims, write_size=False)
            buf, rr = reference.compress_raw(codec, d, ndims, write_size=False)
            assert ro == rr and np.array_equal(buf[:so.size], so)


def test_long_runs_and_run_cap(oracle, reference):
    """runs > 127 blocks (2-byte varint) and > 32767 blocks (cap, sprintz_xff_rle.cpp:71,455)"""
    for esz, codec, nd in [(1, "delta", 5), (2, "xff", 8), (1, "xff", 2), (2, "delta", 1)]:
        for nblocks in (130, 32767 + 5, 70000):
            n = nblocks * 8 * nd + 3
            d = np.zeros(n, np.uint8 if esz == 1 else np.uint16)
            d[-2:] = 7
            _check(oracle, reference, codec, d, nd)


def test_big_stream(oracle, reference):
    """1024*1024+7 elements, as compress_testing.hpp:462"""
    rng = np.random.default_rng(9)
    n = 1024 * 1024 + 7
    for esz, codec, nd in [(1, "xff", 8), (2, "xff", 8), (2, "delta", 32), (1, "delta", 1)]:
        _check(oracle, reference, codec, gen_walk(rng, n, nd, esz, 8, flat_every=5), nd)


@pytest.mark.parametrize("w,ndims", [(8, 1), (8, 3), (8, 8), (8, 80), (16, 1), (16, 2)])
@pytest.mark.parametrize("runs", [True, False])
def test_fire_counters_through_their_wrap(oracle, reference, w, ndims, runs):
    """tests/fire_drive.py: the 8-bit counter through its int16 wrap in both directions, the 16-bit low-dim coefficient past 2^23, with and
    without run spans at the frozen extreme coefficients -- compress bytes and return value, and the reference DECODER's samples (_check).
    (16-bit general FIRE is left out: its reference decoder does not invert runs -- OPT_REF_DECODER_QUIRK, pinned above -- and its truncated
    coefficient has 16 values, all covered by the families)"""
    import fire_drive as fd
    for seed, pattern in ((0, 2), (1, 3)):
        x, ctr = fd.chunk(w, ndims, seed, pattern, runs=None if runs else ())
        if w == 8:
            assert fd.wraps(ctr).any(axis=0).all()
        else:
            assert np.abs(fd.coefficient(ctr, 16, True)).max() > (1 << 23)
        data = np.ascontiguousarray(x).ravel()
        _check(oracle, reference, "xff", data, ndims)
        dr, drr = reference.decompress("xff", oracle.compress("xff", data, ndims)[0], w // 8, data.size, ndims)
        assert drr == data.size and np.array_equal(dr, data)          # (no divergence is legal here: low-dim or 8 bits)


@pytest.mark.parametrize("ndims", [1, 8, 33])
def test_fire_transform_counters_through_their_wrap(oracle, reference, ndims):
    """the stand-alone transform's forecaster (predict.cpp:140-202) on inputs steered against ITS forecast: containers, return values, and back"""
    import fire_drive as fd
    if not reference.has_transforms():
        pytest.skip("oracle/_ref built without the transforms")
    x = fd.transform_input(ndims)
    co, ro = oracle.transform_encode(2, x, ndims)
    cr, rr = reference.transform_encode(2, x, ndims)
    assert ro == rr and np.array_equal(co, cr)
    back, bret = reference.transform_decode(2, co, 1)
    assert bret == x.size and np.array_equal(back, x)


@pytest.mark.parametrize("kind", [0, 1, 3, 4])
def test_steered_online_inputs(orc, reference, kind):
    """tests/online_drive.py past the 64th chain-tile edge (66 tiles of 8 192 blocks) and two periods of the sprintzpack widths: the compiled
    reference's *_pack_u16 writes the oracle's bytes and its decoder restores the input (the smaller plans: tests/test_online_drive_cpu.py)"""
    import online_drive as od
    if kind <= 1:
        x = od.dyndelta_input(od.PLAN_MANY(66), 11, 3)
    else:
        x = od.pack_input(2, 2 * od.PACK_PERIOD + 77, zig=kind == 4, tail=7)
    got, ret, _ = oracle_pack(orc, kind, x)
    if kind <= 1:
        bits = od.choice_bits(got, x.size)
        assert od.longest_dd_run(bits) >= 8192 and bits[64 * 8192 - 1] == 1 and bits[64 * 8192] == 1
    od.reference_agrees(reference.lib, kind, x, got, ret)


@pytest.mark.parametrize("w,ndims", [(8, 1), (8, 5), (8, 8), (16, 2), (16, 8)])
@pytest.mark.parametrize("codec", ["delta", "xff"])
def test_run_drive(oracle, reference, codec, w, ndims):
    """tests/rle_drive.py: every chunk of the five batches that steer the RLE / group state machine (run lengths 1 .. 16 and 126 .. 129
    closing in both slots, roll-overs, runs at the stream's start and end, the padding slot), at chunk lengths of whole blocks and
    1 and 8 D - 1 elements more, and the cap -- the compiled reference writes the oracle's bytes (_check: and decodes them)"""
    import rle_drive as rd
    for kind in rd.KINDS:
        for r in (0, 1, 8 * ndims - 1):
            x, chunk_len, _ = rd.batch(codec, w, ndims, kind, 16, 256, r)
            for c in range(16):
                _check(oracle, reference, codec, x[c * chunk_len:(c + 1) * chunk_len], ndims)
    if (w, ndims) in ((8, 1), (8, 5)):
        x, chunk_len, _ = rd.cap_chunks(codec, w, ndims, nchunks=1)
        _check(oracle, reference, codec, x, ndims)
