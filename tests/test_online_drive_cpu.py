"""CPU tier of the steered "online" inputs (tests/online_drive.py): the coverage they exist for is asserted on the ORACLE's containers (what the
encoder chose, never what the plan asked for), under both losses; the oracle inverts them, the model written from the format decodes them,
the golden set minted from the compiled reference (oracle/gen_golden_online_drive.py) has the oracle's bytes, and -- where oracle/_ref exists --
so does the compiled reference itself.

The four (choice before, choice after) pairs at multiples of 8 192 need at least six chain-tile edges once a run of 3 x 8 192 + 700 blocks
holds three of them as (1,1): PLAN_SMALL (4.4 tiles, the size the model and the stored container are meant for) has (0,1) and (1,1) there and
all four pairs at 4, 16, 256 and 1 024; PLAN_MANY has all four at every size, 8 192 included, and is what the GPU tier runs past one tile."""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

import online_drive as od
from harness import REF_SO
from codec_helpers import oracle_pack, oracle_unpack, orc  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_PAIRS = {(0, 0), (0, 1), (1, 0), (1, 1)}
MANY_TILES = 66            # past the 64th tile edge


@pytest.fixture(scope="module")
def golden_online_drive():
    gdir = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gdir, "golden_online_drive_v1.json")) as f:
        manifest = json.load(f)["cases"]
    return manifest, np.load(os.path.join(gdir, "golden_online_drive_v1.npz"))


@pytest.fixture(scope="module")
def many(orc):
    """PLAN_MANY(66) and the oracle's containers of it under both losses"""
    x = od.dyndelta_input(od.PLAN_MANY(MANY_TILES), 11, 3)
    return x, {kind: oracle_pack(orc, kind, x)[0] for kind in (0, 1)}


@pytest.mark.parametrize("kind", [0, 1])
def test_small_plan_reaches_what_it_is_for(orc, kind):
    for tail in range(8):
        x = od.small_input(tail)
        assert x.size == 1 + 8 * od.SMALL_BLOCKS + tail
        cont, ret, _ = oracle_pack(orc, kind, x)
        bits = od.choice_bits(cont, x.size)
        assert bits.size == od.SMALL_BLOCKS
        assert od.longest_dd_run(bits) >= 3 * 8192 + 700                   # m = 8 x count wraps 2^16 three times inside one run
        for B in (4, 16, 256, 1024):
            assert od.pairs_at(bits, B) == ALL_PAIRS, (B, tail)
        assert od.pairs_at(bits, 8192) >= {(0, 1), (1, 1)}                # (see the module's docstring; all four: PLAN_MANY below)
        assert bits[0] == 1                                                # double delta from the first block on: d enters as 0
        assert len(od.whole_dd_tiles_with_d(cont, x.size)) >= 3           # chain tiles that are a = 1 as a whole, d != 0 entering
        assert od.has_zigzag_ffff(cont, x.size)
        vals, _, lens = od.run_lengths(bits)
        assert ((vals == 0) & (lens == 1)).sum() >= 3 and ((vals == 1) & (lens == 1)).sum() >= 3   # single blocks of either kind inside runs of the other
        back, dret = oracle_unpack(orc, kind, cont, x.size)
        assert dret == x.size and np.array_equal(back, x)
        assert np.array_equal(od.dyndelta_model(cont, x.size), x)


def test_the_encoder_follows_the_plan(orc):
    """the steering itself: outside the extremes (where the encoder may pick either) every block got the planned predictor under both losses"""
    for plan, x in ((od.PLAN_SMALL, od.small_input(0)), (od.plan_blocks(3 * 8192 + 1), od.blocks_input(3 * 8192 + 1, 5, 7))):
        lab = od.labels_of_plan(plan)
        for kind in (0, 1):
            bits = od.choice_bits(oracle_pack(orc, kind, x)[0], x.size)
            assert np.array_equal(bits[lab != od.X], lab[lab != od.X]), kind


@pytest.mark.parametrize("kind", [0, 1])
def test_many_plan_has_every_pair_at_every_boundary(orc, many, kind):
    x, conts = many
    cont = conts[kind]
    bits = od.choice_bits(cont, x.size)
    assert bits.size == MANY_TILES * 8192
    for B in od.BOUNDARIES:
        assert od.pairs_at(bits, B) == ALL_PAIRS, B
    assert bits[64 * 8192 - 1] == 1 and bits[64 * 8192] == 1               # a run across the 64th tile edge
    assert od.whole_dd_tiles_with_d(cont, x.size)
    assert od.has_zigzag_ffff(cont, x.size)
    back, dret = oracle_unpack(orc, kind, cont, x.size)
    assert dret == x.size and np.array_equal(back, x)
    assert np.array_equal(od.dyndelta_model(cont, x.size), x)


def test_many_plan_runs_across_the_512th_edge():
    lab = od.labels_of_plan(od.PLAN_MANY(515))
    assert lab.size == 515 * 8192
    assert (lab[511 * 8192:512 * 8192 + 200] == od.DD).all()               # (the plan only: the GPU tier's inputs of this size assert it on the container)


def test_model_agrees_with_its_slow_form(orc):
    x = od.blocks_input(2600, 3, 6)
    for kind in (0, 1):
        cont, _, _ = oracle_pack(orc, kind, x)
        assert np.array_equal(od.dyndelta_model_slow(cont, x.size), x)
        assert np.array_equal(od.dyndelta_model(cont, x.size), x)


@pytest.mark.parametrize("kind", [3, 4])
def test_pack_input_gives_every_width_a_tile(orc, kind):
    x = od.pack_input(od.GOLDEN_SEED, od.PACK_SMALL_BLOCKS, zig=kind == 4, tail=3)
    cont, ret, _ = oracle_pack(orc, kind, x)
    nib = od.pack_nibbles(cont, x.size)
    w = od.pack_widths(od.GOLDEN_SEED, od.PACK_SMALL_BLOCKS)
    assert np.array_equal(nib, np.where(w == 16, 15, w))                   # widths 15 and 16 both give nibble 15
    assert od.nibbles_owning_a_tile(nib) == set(range(16))                 # 1 024 aligned blocks in a row of every nibble
    pay = od.tile_payloads(nib)
    assert pay.min() == 0 and pay.max() == 16 * 1024
    mixed, wm = nib[od.PACK_STRETCH:od.PACK_STRIDE], w[od.PACK_STRETCH:od.PACK_STRIDE]
    assert (wm[1:256] != wm[:255]).all() and (wm[257:] != wm[256:-1]).all()   # the width changes every block (the nibbles are the widths: above)
    assert ((mixed[:-1] == 15) & (mixed[1:] <= 2)).sum() >= 100            # escape blocks next to narrow ones
    back, dret = oracle_unpack(orc, kind, cont, x.size)
    assert dret == x.size and np.array_equal(back, x)


def test_oracle_matches_golden(orc, golden_online_drive):
    manifest, arrays = golden_online_drive
    cases = {name: (kind, x) for name, kind, x in od.golden_cases()}
    assert set(cases) == {m["name"] for m in manifest}
    stored = 0
    for m in manifest:
        kind, x = cases[m["name"]]
        assert kind == m["kind"] and x.size == m["n"] and zlib.crc32(x.tobytes()) == m["input_crc32"], m["name"]
        got, ret, _ = oracle_pack(orc, kind, x)
        assert ret == m["ret"] and got.size == m["nbytes"] and zlib.crc32(got.tobytes()) == m["container_crc32"], m["name"]
        if m["stored"]:
            assert np.array_equal(got, arrays[m["name"]])
            stored += 1
    assert stored == 2


@pytest.mark.parametrize("kind", [0, 1, 3, 4])
def test_oracle_matches_compiled_reference(orc, kind):
    """every golden case's input and a plan of 8 chain tiles against the compiled reference itself"""
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref not built (reference sources absent)")
    if kind <= 1:
        xs = [od.small_input(t) for t in range(8)] + [od.dyndelta_input(od.PLAN_MANY(8), 21, 2)]
    else:
        xs = [od.pack_input(s, od.PACK_SMALL_BLOCKS, zig=kind == 4, tail=t) for s, t in ((0, 3), (1, 0))]
    ref = C.CDLL(REF_SO)
    for x in xs:
        od.reference_agrees(ref, kind, x, *oracle_pack(orc, kind, x)[:2])
