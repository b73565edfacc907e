"""CPU tier of the FIRE counter extremes: tests/fire_drive.py steers the forecaster's counters through the int16 wrap of the 8-bit codec
(reference util.h:39-47; _mm256_add_epi16 in sprintz_xff_rle.cpp:1067, sprintz_xff_lowdim.cpp:965, predict.cpp:202) and the 16-bit low-dim
coefficient past 2^23, where a 24-bit multiply no longer holds it.  Here: the generator gets where it says (coverage, from its own model of
the counters, which agrees with kat.fire_coefficients), the oracle inverts its own streams of these inputs, and the oracle's streams are the
compiled reference's (tests/golden/golden_firewrap_v1, minted by oracle/gen_golden_firewrap.py; tests/test_oracle_vs_ref.py where the
reference is built).  The GPU tier (tests/test_gpu_fire_extremes.py) runs every kernel family on the same inputs."""
import json
import os
import zlib

import numpy as np
import pytest

import fire_drive as fd
import kat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_firewrap_v1")


def load_golden():
    with open(GOLDEN + ".json") as f:
        manifest = json.load(f)["cases"]
    return manifest, np.load(GOLDEN + ".npz")


def counters_of(w, ncols, transform=False):
    """the counters of the batch's first four chunks side by side: both alternating patterns, all up, all down"""
    return np.concatenate([fd.chunk(w, ncols, k, (2, 3, 0, 1)[k], transform=transform)[1] for k in range(4)], axis=1)


@pytest.mark.parametrize("ncols,transform", [(1, False), (4, False), (8, False), (80, False), (8, True)])
def test_every_8_bit_counter_wraps(ncols, transform):
    """a block moves a counter by 32 at most: a jump of more than 30 000 between two blocks is the int16 wrap"""
    ctr = counters_of(8, ncols, transform)
    jump = np.diff(ctr, axis=0)
    assert (np.abs(ctr) <= 32768).all()
    assert fd.wraps(ctr).any(axis=0).all(), "a column never wrapped"
    assert (jump < -30000).any() and (jump > 30000).any(), "wraps in one direction only"
    assert (np.abs(jump)[~fd.wraps(ctr)] <= 32).all()


def test_general_layout_visits_every_coefficient():
    """sprintz_xff_rle.cpp:217 at 8 bits: int16((ctr >> 5) << 4) -- all 2 048 multiples of 16 in [-16 384, 16 368]; the transform's too"""
    for transform in (False, True):
        co = fd.coefficient(counters_of(8, 8, transform), 8, False)
        assert set(np.unique(co).tolist()) == set(range(-16384, 16384, 16))


def test_low_dim_coefficients_reach_both_ends():
    co = fd.coefficient(counters_of(8, 4), 8, True)                  # sprintz_xff_lowdim.cpp:170-173: ctr >> 1, untruncated
    assert co.min() <= -16000 and co.max() >= 16000, (co.min(), co.max())
    for ncols in (1, 2):
        co = fd.coefficient(counters_of(16, ncols), 16, True)
        # beyond 2^23 the coefficient does not fit the 24-bit multiply the kernels use everywhere else (sprintz_device.h, fire_predict)
        assert co.min() < -(1 << 23) and co.max() > (1 << 23), (ncols, co.min(), co.max())


@pytest.mark.parametrize("w,ncols", [(8, 1), (8, 8), (16, 2)])
def test_run_spans_sit_at_extreme_coefficients(w, ncols):
    """run blocks replay the forecast with the frozen coefficient: one span where it is large, one behind a wrap (8 bits)"""
    runs = fd.RUNS8 if w == 8 else fd.RUNS16
    assert sum(b - a for a, b in runs) <= 60
    ctr = counters_of(w, ncols)
    co = fd.coefficient(ctr, w, fd.is_lowdim(w, ncols))
    in_run = np.zeros(ctr.shape[0], bool)
    for a, b in runs:
        in_run[a:b] = True
        assert (ctr[a:b + 1] == ctr[a]).all(), "counters only move on real blocks"
    assert (np.abs(co[in_run]) >= (8192 if w == 8 else 1 << 23)).any()
    if w == 8:
        wrapped = np.cumsum(np.vstack([np.zeros((1, ctr.shape[1]), bool), fd.wraps(ctr)]), axis=0) > 0
        first = int(np.argmax(wrapped.any(axis=1)))              # the block that starts with the first wrapped counter
        assert wrapped[in_run].any(), "no run block behind a wrap"
        assert any(a < first and (np.abs(co[a:b]) >= 8192).any() for a, b in runs), "no run at a large coefficient before the first wrap"
        assert any(first <= a <= first + 10 for a, _ in runs), "no run within 10 blocks of the first wrap"


@pytest.mark.parametrize("w,ncols", [(8, 1), (8, 3), (8, 8), (8, 64), (16, 1), (16, 2)])
def test_model_agrees_with_kat(w, ncols):
    x, ctr = fd.chunk(w, ncols, 1, 3)
    low = fd.is_lowdim(w, ncols)
    want = np.stack(kat.fire_coefficients(x[None], w, low))[:, 0, :]
    assert np.array_equal(fd.coefficient(ctr, w, low), want)


@pytest.mark.parametrize("w,ncols", [(8, 1), (8, 2), (8, 3), (8, 4), (8, 8), (8, 80), (16, 1), (16, 2)])
def test_oracle_round_trip(oracle, w, ncols):
    for seed, pattern in ((0, 2), (1, 3), (2, 0), (3, 1)):
        x = fd.codec_input(w, ncols, seed, pattern)
        s, r = oracle.compress("xff", x, ncols)
        d, dr = oracle.decompress("xff", s, w // 8, x.size)
        assert dr == x.size and np.array_equal(d, x), (seed, pattern)


def test_wide_inputs_are_tiles(oracle):
    """600 and 2 048 columns: 64 trajectories, tiled -- columns are independent and the run spans common, so every column still does its part"""
    for ncols in (600, 2048):
        x, ctr = fd.chunk(8, ncols, 0, 2)
        assert x.shape == (8 * fd.NB8, ncols) and np.array_equal(x[:, :64], x[:, 64:128]) and np.array_equal(x[:, :ncols % 64 or 64], x[:, -(ncols % 64 or 64):]) and fd.wraps(ctr).any(axis=0).all()
    x = np.ascontiguousarray(fd.chunk(8, 600, 0, 2)[0]).ravel()
    s, _ = oracle.compress("xff", x, 600)
    d, dr = oracle.decompress("xff", s, 1, x.size)
    assert dr == x.size and np.array_equal(d, x)


@pytest.mark.parametrize("ncols", [1, 8, 33])
def test_transform_model_is_the_oracles(oracle, ncols):
    """the errors the generator's model of the stand-alone transform computes are oracle.transform_encode's on every forecast block (the blocks
    behind them are plain deltas by design, transforms_oracle.c:62-72), and the oracle inverts its container"""
    x = fd.transform_input(ncols)
    errs = fd.drive(8, False, fd.directions(fd.TILE, fd.GOLDEN_PATTERN), fd.GOLDEN_SEED, fd.NB8, fd.RUNS8, True)[2][:, :ncols]
    cont, ret = oracle.transform_encode(2, x, ncols)
    nfore = fd.transform_forecast_blocks(x.size, ncols)
    assert 0 < fd.NB8 - nfore <= 4 and ret == x.size + 6
    m = nfore * 8 * ncols
    assert np.array_equal(cont[6:6 + m], errs.ravel()[:m])
    prev = np.concatenate([x[m - ncols:m], x[m:-ncols]]) if x.size - m > ncols else x[m - ncols:x.size - ncols]
    assert np.array_equal(cont[6 + m:], (x[m:] - prev).astype(np.uint8))
    back, bret = oracle.transform_decode(2, cont, 1)
    assert bret == x.size and np.array_equal(back, x)


def test_golden_streams_are_the_oracles(oracle):
    """the fixture pins the generator (CRC32 of every input) and holds the oracle to the compiled reference's bytes"""
    manifest, arrays = load_golden()
    assert [(m["w"], m["ndims"]) for m in manifest if m["what"] == "codec"] == list(fd.GOLDEN_CODEC)
    assert [(m["w"], m["ndims"]) for m in manifest if m["what"] == "transform"] == list(fd.GOLDEN_TRANSFORM)
    for m in manifest:
        if m["what"] == "codec":
            x = fd.codec_input(m["w"], m["ndims"])
            got, ret = oracle.compress("xff", x, m["ndims"])
        else:
            x = fd.transform_input(m["ndims"])
            got, ret = oracle.transform_encode(2, x, m["ndims"])
        assert x.size == m["n"] and zlib.crc32(x.tobytes()) == m["input_crc32"], (m, "the generator's output changed")
        assert ret == m["ret"] and np.array_equal(got, arrays[m["name"]]), m
