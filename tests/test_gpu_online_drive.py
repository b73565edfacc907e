"""GPU tier of the steered "online" inputs (tests/online_drive.py; coverage asserted in tests/test_online_drive_cpu.py): the dynamic-delta
decoders' scans (sprintz_amd/csrc/online.hip: dyndelta_chain_kernel, dyndelta_tile / tilescan / decode_kernel) and sprintzpack's offset scan
(tile_offsets_kernel) where their state crosses lanes, waves, tiles, tickets and slabs -- on inputs whose double-delta runs are longer than
each of those units, at the smallest sizes that reach each loop:

  PLAN_SMALL (36 240 blocks)                      every boundary up to the chain tile, m wrapping 2^16; both forms; every tail
  127 x 8 192 and 127 x 8 192 + 1 blocks          the default threshold between the three-launch and the one-pass form, no setting
  max(2 CUs + 3, 515) chain tiles                 workgroups take second and third tickets, waves 1 .. 7 look back; as three launches: more than
                                                  4 096 tiles, the tile scan's second slab
  1 024 x 8 192 + 1 029 blocks                    as three launches: more than 8 192 tiles, the tile scan's third slab -- the first whose carry is
                                                  a composition of two slab totals
  8 192 x 1 024 + 3 x 1 024 + 5 sprintzpack blocks   tile_offsets_kernel's second slab, pack and unpack
  n around 2 Mi                                   the host single calls on both sides of the pinned buffer's 4 MiB

Every device case (roundtrip): pack == the oracle's bytes and return value (and the golden CRC32 minted from the compiled reference where the case
is in that set), unpack == the input; d_tmp exactly online_tmp_bytes long, pre-filled with 0xA5 and NOT cleared between the calls; guard bytes
behind dest (online_bound bytes) and out (n samples) untouched; a second unpack under the other form with the same d_tmp.  (Sprintzpack has
one form: there the second unpack is the same call again, and what it checks is that a d_tmp left dirty by pack and unpack is reusable.)"""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

import online_drive as od
from dispatch import ran
from codec_helpers import oracle_pack, orc  # noqa: F401  (fixtures)
from fixtures import lib  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = "SPRINTZ_MI355X_ONLINE_CHAIN"
GUARD = 256                    # bytes behind dest, and behind out
CHAIN, THREE = dict(on_chain=1, on_three=0), dict(on_chain=0, on_three=1)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "golden_online_drive_v1.json")) as f:
        manifest = {m["name"]: m for m in json.load(f)["cases"]}
    return manifest, np.load(os.path.join(ROOT, "tests", "golden", "golden_online_drive_v1.npz"))


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def to_device(x):
    """uint16 samples -> int16 device tensor (the inputs are read-only arrays, hence the copy)"""
    import torch
    return torch.from_numpy(np.array(x, copy=True).view(np.int16)).cuda()


def set_form(monkeypatch, value):
    if value is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, value)


def roundtrip(lib, monkeypatch, kind, x, want, wret, forms, golden_case=None):
    """forms: ((setting or None, expected dispatch), ...) of the unpack calls, in order; all share one d_tmp"""
    import torch
    n = x.size
    bound, tmpb = int(lib.online_bound(kind, n)), int(lib.online_tmp_bytes(kind, n))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dx = to_device(x)
    dest = torch.full((bound + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    tmp = torch.full((tmpb,), 0xA5, dtype=torch.uint8, device="cuda")
    ret = torch.full((1,), -77, dtype=torch.int64, device="cuda")
    lib.check(lib.online_pack_device(kind, dx.data_ptr(), n, dest.data_ptr(), ret.data_ptr(), tmp.data_ptr(), st))
    r = int(ret.item())
    assert r == wret, (kind, n, r, wret)
    assert torch.equal(dest[: 2 * r], torch.from_numpy(want).cuda()), (kind, n, "container differs from the oracle's")
    assert bool((dest[bound:] == 0x5A).all()), (kind, n, "pack wrote behind online_bound bytes")
    if golden_case is not None:
        manifest, arrays = golden_case[0]
        m = manifest[golden_case[1]]
        got = dest[: 2 * r].cpu().numpy()
        assert m["n"] == n and m["ret"] == r and m["nbytes"] == got.size and zlib.crc32(got.tobytes()) == m["container_crc32"], m["name"]
        if m["stored"]:
            assert np.array_equal(got, arrays[m["name"]]), m["name"]
    for setting, expect in forms:
        set_form(monkeypatch, setting)
        out = torch.full((n + GUARD // 2,), 0x7B7B, dtype=torch.int16, device="cuda")
        ret.fill_(-77)
        with ran(**expect):
            lib.check(lib.online_unpack_device(kind, dest.data_ptr(), n, out.data_ptr(), ret.data_ptr(), tmp.data_ptr(), st))
        assert int(ret.item()) == n, (kind, n, setting)
        assert torch.equal(out[:n], dx), (kind, n, setting, "samples differ from the input")
        assert bool((out[n:] == 0x7B7B).all()), (kind, n, setting, "unpack wrote behind n samples")
        assert bool((dest[bound:] == 0x5A).all())


def forms_for(kind, chain, chain_runs):
    """the first unpack under the parametrised setting, the second under the other form.  chain_runs: the default setting takes the one-pass form.
    Kinds 3 and 4 have a single form (neither counter moves): the same call twice, the second on the d_tmp the first left dirty"""
    if kind > 1:
        return ((None, dict(on_chain=0, on_three=0)),) * 2
    first = CHAIN if chain == "1" or (chain == "default" and chain_runs) else THREE
    second = THREE if first is CHAIN else CHAIN
    return ((None if chain == "default" else chain, first), ("0" if second is THREE else "1", second))


# ------------------------------------------------------------------------------------------------ 1. PLAN_SMALL
@pytest.mark.parametrize("chain", ["1", "0", "default"])
@pytest.mark.parametrize("kind", [0, 1])
def test_small_plan_every_tail(lib, orc, golden, monkeypatch, kind, chain):
    """4.4 chain tiles, 35.4 three-launch tiles; a double-delta run of 25 276 blocks and runs that start and end one block before, on and after
    the multiples of 4, 16, 256, 1 024 and 8 192; 0 .. 7 trailing elements.  The default setting takes the three-launch form (fewer than 128 tiles)"""
    for tail in range(8):
        x = od.small_input(tail, od.GOLDEN_SEED)
        want, wret, _ = oracle_pack(orc, kind, x)
        roundtrip(lib, monkeypatch, kind, x, want, wret, forms_for(kind, chain, False), (golden, f"small_k{kind}_t{tail}"))


@pytest.mark.parametrize("kind", [3, 4])
def test_small_pack_every_width(lib, orc, golden, monkeypatch, kind):
    """every width 0 .. 16 owning a whole tile (payload 0 and 16 x 1 024 among them), then widths that change every block"""
    x = od.pack_input(od.GOLDEN_SEED, od.PACK_SMALL_BLOCKS, zig=kind == 4, tail=3)
    want, wret, _ = oracle_pack(orc, kind, x)
    roundtrip(lib, monkeypatch, kind, x, want, wret, forms_for(kind, None, False), (golden, f"pack_k{kind}"))


# ------------------------------------------------------------------------------------------------ 2. the default threshold
@pytest.mark.parametrize("nblocks,first", [(127 * 8192, THREE), (127 * 8192 + 1, CHAIN)])
def test_default_threshold(lib, orc, monkeypatch, nblocks, first):
    """no setting: 127 chain tiles decode in three launches, one block more (128 tiles) in one pass -- on steered data (8.3 Mi samples)"""
    x = od.blocks_input(nblocks, 31, 3)
    want, wret, _ = oracle_pack(orc, 0, x)
    bits = od.choice_bits(want, x.size)
    assert bits.size == nblocks and od.pairs_at(bits, 8192) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    second = CHAIN if first is THREE else THREE
    roundtrip(lib, monkeypatch, 0, x, want, wret, ((None, first), ("1" if second is CHAIN else "0", second)))


# ------------------------------------------------------------------------------------------------ 3. more tiles than workgroups, two slabs of tiles
@pytest.fixture(scope="module")
def many(orc, cus):
    """PLAN_MANY(max(2 CUs + 3, 515)) with 5 trailing elements, generated once; the oracle's containers per kind on demand, kept"""
    tiles = max(2 * cus + 3, 515)
    x = od.dyndelta_input(od.PLAN_MANY(tiles), 41, 5)
    conts = {}

    def cont(kind):
        if kind not in conts:
            conts[kind] = oracle_pack(orc, kind, x)[:2]
        return conts[kind]
    return tiles, x, cont


@pytest.mark.parametrize("chain", ["default", "0"])
@pytest.mark.parametrize("kind", [0, 1])
def test_more_tiles_than_workgroups(lib, monkeypatch, many, cus, kind, chain):
    """default: one pass, at least 2 CUs + 3 tiles on a grid of one workgroup a CU -- second and third tickets, look-back windows of waves 1 .. 7
    (the first cohort's predecessors are maps, not states); "0": more than 4 096 three-launch tiles -- the tile scan's second slab"""
    tiles, x, cont = many
    want, wret = cont(kind)
    bits = od.choice_bits(want, x.size)
    assert bits.size == tiles * 8192 > 2 * cus * 8192 and bits.size // 1024 > 4096
    assert bits[512 * 8192 - 8392:512 * 8192 + 200].all()                  # the run across the 512th edge, tile 511 as a whole
    assert od.pairs_at(bits, 8192) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    roundtrip(lib, monkeypatch, kind, x, want, wret, forms_for(kind, chain, True))


THREE_SLABS_BLOCKS = 1024 * 8192 + 1029


def test_three_slabs_of_tiles(lib, orc, monkeypatch):
    """"0": 8 194 three-launch tiles.  The tile scan takes 4 096 tiles a slab, and what it carries from slab to slab first differs from the
    last slab's total alone in front of the THIRD slab (in front of the second the carry is the first slab's total either way) -- so the
    accumulation `carry = compose(carry, total)` needs more than 8 192 tiles: 1 025 chain tiles, 67 Mi samples.  The run across the 1 024th
    chain-tile edge makes the third slab's tiles double delta throughout: they take x AND d from the carry.  Then the one-pass form on the same
    container: its fourth and fifth tickets on a 256-CU part"""
    x = od.blocks_input(THREE_SLABS_BLOCKS, 47, 3)
    want, wret, _ = oracle_pack(orc, 0, x)
    bits = od.choice_bits(want, x.size)
    assert bits.size == THREE_SLABS_BLOCKS and -(-bits.size // 1024) > 2 * 4096
    assert bits[1023 * 8192 - 200:].all() and x[8 * 8192 * 1024] != x[8 * 8192 * 1024 - 1]     # a = 1 from tile 1 023 on, d != 0 entering the third slab
    roundtrip(lib, monkeypatch, 0, x, want, wret, (("0", THREE), ("1", CHAIN)))


# ------------------------------------------------------------------------------------------------ 4. sprintzpack past one slab of tile sums
PACK_BIG_BLOCKS = 8192 * 1024 + 3 * 1024 + 5


@pytest.fixture(scope="module")
def pack_big():
    """kind 3's input, generated once; kind 4's is the same magnitudes with the zigzag undone"""
    x3 = od.pack_input(51, PACK_BIG_BLOCKS, zig=False, tail=3)
    v = x3.astype(np.int32)
    return {3: x3, 4: (((v >> 1) ^ -(v & 1)) & 0xffff).astype(np.uint16)}


@pytest.mark.parametrize("kind", [3, 4])
def test_pack_past_one_slab(lib, orc, monkeypatch, pack_big, kind):
    """8 196 tiles of 1 024 blocks: the offsets of the last four come from tile_offsets_kernel's second slab (its 64-bit carry), packing and unpacking"""
    x = pack_big[kind]
    want, wret, _ = oracle_pack(orc, kind, x)
    assert x.size // 8 == PACK_BIG_BLOCKS and -(-PACK_BIG_BLOCKS // 1024) > 8192
    assert od.tile_payloads(od.pack_nibbles(want, x.size))[8192:].sum() > 0  # the second slab's tiles carry payload
    roundtrip(lib, monkeypatch, kind, x, want, wret, forms_for(kind, None, False))


# ------------------------------------------------------------------------------------------------ 5. two one-pass decodes in flight
def test_two_chain_decodes_in_flight(lib, monkeypatch, many):
    """like test_one_pass_decoders_on_two_streams_at_once (tests/test_gpu_transforms.py): the one-pass decoder's workgroups wait for each other;
    with two decodes in flight on two streams neither has the chip to itself -- a waiting tile's predecessors are held by running workgroups --
    and both must finish and be right, three decodes each"""
    import torch
    set_form(monkeypatch, None)
    tiles, xa, _ = many
    xb = od.dyndelta_input(od.PLAN_MANY(tiles), 43, 2)
    dev = torch.device("cuda:0")
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    cur = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    xs, conts, tmps, rets, outs = [], [], [], [], [[], []]
    for k, x in enumerate((xa, xb)):
        n = x.size
        dx = to_device(x)
        dest = torch.zeros(int(lib.online_bound(k, n)), dtype=torch.uint8, device="cuda")
        tmp = torch.full((int(lib.online_tmp_bytes(k, n)),), 0xA5, dtype=torch.uint8, device="cuda")
        ret = torch.zeros(1, dtype=torch.int64, device="cuda")
        lib.check(lib.online_pack_device(k, dx.data_ptr(), n, dest.data_ptr(), ret.data_ptr(), tmp.data_ptr(), cur))      # kind 0 for the first, 1 for the second
        xs.append(dx), conts.append(dest), tmps.append(tmp), rets.append([torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(3)])
    torch.cuda.synchronize()
    with ran(on_chain=6, on_three=0):
        for it in range(3):
            for k in range(2):
                with torch.cuda.stream(streams[k]):
                    out = torch.zeros(xs[k].numel() + 16, dtype=torch.int16, device="cuda")
                    outs[k].append(out)
                    lib.check(lib.online_unpack_device(k, conts[k].data_ptr(), xs[k].numel(), out.data_ptr(), rets[k][it].data_ptr(), tmps[k].data_ptr(),
                                                       C.c_void_p(streams[k].cuda_stream)))
    torch.cuda.synchronize()
    for k in range(2):
        for it in range(3):
            assert int(rets[k][it].item()) == xs[k].numel(), (k, it)
            assert torch.equal(outs[k][it][: xs[k].numel()], xs[k]), (k, it)


# ------------------------------------------------------------------------------------------------ 6. host single calls around the pinned buffer's 4 MiB
PIN_MAX = 4 << 20


def largest_n_with_bound_pinned(lib, kind):
    n = PIN_MAX // 2
    while int(lib.online_bound(kind, n)) > PIN_MAX:
        n -= 1
    return n


@pytest.mark.parametrize("which", ["both", "mixed-9", "mixed", "neither"])
@pytest.mark.parametrize("kind", [0, 2, 3])
def test_host_calls_on_both_sides_of_the_pinned_buffer(lib, orc, kind, which):
    """online_pack / online_unpack stage transfers of at most 4 MiB through the pinned buffer and send larger ones straight from / to the caller's
    memory, the input and the output each on its own: "both" is the largest n whose online_bound still fits (2 n is far below), 2 Mi - 9 and
    2 Mi (2 n <= 4 MiB < online_bound; 2 Mi: 2 n == 4 MiB exactly) mix the two, 2 Mi + 9 pins neither.  The unpack's input is the container
    (4 + 2 n + ... bytes), its output 2 n bytes.  Bytes and return values against the oracle; nothing written past 2 ret bytes / n samples;
    the container handed to the unpack is not a byte longer than it is"""
    n = {"both": largest_n_with_bound_pinned(lib, kind), "mixed-9": (2 << 20) - 9, "mixed": 2 << 20, "neither": (2 << 20) + 9}[which]
    bound = int(lib.online_bound(kind, n))
    assert (2 * n <= PIN_MAX, bound <= PIN_MAX) == {"both": (True, True), "mixed-9": (True, False), "mixed": (True, False), "neither": (False, False)}[which]
    if kind == 0:
        x = od.blocks_input((n - 1) // 8, 61, (n - 1) % 8)
    elif kind == 2:
        x = np.random.default_rng(62).integers(0, 1 << 16, size=n).astype(np.uint16)
        x[:6] = (0, 0x8000, 0xffff, 0x7fff, 1, 0x8001)
    else:
        x = od.pack_input(63, n // 8, tail=n % 8)
    assert x.size == n
    want, wret, _ = oracle_pack(orc, kind, x)
    dest = np.full(bound + GUARD, 0x5A, np.uint8)
    ret = int(lib.online_pack(kind, x.ctypes.data, n, dest.ctypes.data))
    assert ret == wret, (lib.last_error(), ret, wret)
    assert np.array_equal(dest[: 2 * ret], want)
    assert (dest[2 * ret:] == 0x5A).all()
    cont = want.copy()                                                     # exactly the container
    out = np.full(n + 64, 0x7B7B, np.uint16)
    dret = int(lib.online_unpack(kind, cont.ctypes.data, out.ctypes.data))
    assert dret == n, (lib.last_error(), dret)
    assert np.array_equal(out[:n], x)
    assert (out[n:] == 0x7B7B).all()
