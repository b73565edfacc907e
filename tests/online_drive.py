"""Inputs that STEER the "online" coders (sprintz_amd/csrc/online.hip; formats: oracle/online_oracle.c's header comment) and a small model of
the dynamic-delta decoder.  Plain numpy; nothing here is product code or oracle code (reference_agrees calls the compiled reference it is given).

Why: a dynamic-delta block is a map on the decoder's state (x, d) = (last value, last difference).  A delta block RESETS d (m = 0, a = 0), a
double-delta block passes d through and adds m d to x (m = 8, a = 1).  The decoders are scans over these maps, and a wrong composition order,
a wrong look-back order or a dropped carry only shows on stretches of double-delta blocks with a non-zero d entering them -- stretches longer
than the unit that has to carry them: a lane of the one-pass decoder (16 blocks), a wave load (256), a three-launch tile / a chain wave
(1 024), a chain tile (8 192), the 2^16 wrap of m (8 192 blocks in a row).  Random walks and noise give runs of at most 18 blocks.

dyndelta_input(plan, seed, tail) builds a stream from (choice, nblocks) segments such that the ENCODER picks the planned predictor for every
block under both losses (the tests assert coverage on the oracle's container, never on the plan):
  DD  double delta: first differences walk inside [100, 500] (reflected), second differences in {-1, 0, 1}: d is never 0, x wraps 2^16 every
      ~ 200 samples, the double-delta errors are 0 / +-1 against delta errors of 100 .. 500
  D   delta: first differences alternate in sign (-, +, -, ...) with magnitudes in [2 000, 3 000]: a double-delta error is the sum of two
      magnitudes, larger than the delta error sample by sample (a tie keeps delta: loss0 <= loss1).  The last difference of a D segment in
      front of a DD segment is that segment's starting difference, so the DD segment is entered smoothly (its first error is 0 / +-1 too)
  X   extremes: samples from {0, 0x8000, 0xffff}, the cycle first, then drawn at random: block sums A and C pass 2^16, zigzag 0xffff
      occurs; whichever predictor the encoder picks.  Ends on 0xffff, 0 (a difference of +1); a D segment must follow
pack_input(seed, nblocks, zig) does the same for sprintzpack's widths."""
from functools import lru_cache

import numpy as np

D, DD, X = 0, 1, 2
T = 8192                       # blocks of a chain tile (online.hip: kDcTileBlocks); a three-launch tile and a chain wave are 1 024
BOUNDARIES = (4, 16, 256, 1024, 8192)


# ------------------------------------------------------------------------------------------------ plans
def plan_of_labels(lab):
    lab = np.asarray(lab, np.int8)
    edges = np.flatnonzero(np.diff(lab)) + 1
    starts = np.concatenate([[0], edges])
    ends = np.concatenate([edges, [lab.size]])
    return tuple((int(lab[a]), int(b - a)) for a, b in zip(starts, ends))


def labels_of_plan(plan):
    return np.repeat(np.array([c for c, _ in plan], np.int8), np.array([k for _, k in plan], np.int64))


# The motifs of ONE chain tile, as block offsets from the tile's first block.  For every boundary size B below the tile: a DD run of B blocks
# that starts and ends one block BEFORE a multiple of B, one ON it, one AFTER it -- so the multiples of B see all four (choice before, choice
# after) pairs (the first 200 and the last 200 blocks of a tile are left to PLAN_MANY's runs at the tile edges) -- then single D blocks inside DD runs and single DD blocks inside D stretches.
_TILE_DD = (
    (515, 519), (524, 528), (533, 537),                  # B = 4:     516: (1,1) 520: (0,0) 524: (0,1)  528: (1,0)
    (543, 559), (576, 592), (609, 625),                  # B = 16:    544: (1,1) 560: (0,0) 576: (0,1)  592: (1,0)
    (255, 511), (768, 1024), (1281, 1537),               # B = 256:   256: (1,1) 512: (0,0) 768: (0,1)  1 024: (1,0)
    (2047, 3071), (4096, 4500), (4501, 5120), (6145, 7169),   # B = 1 024: 2 048: (1,1) 3 072: (0,0) 4 096: (0,1) 5 120: (1,0); a single D block at 4 500
    (2600, 2601), (1700, 1701), (3500, 3501), (5600, 5601), (7500, 7501),   # single DD blocks in D stretches (2 600: no-op, inside a run)
)
_TILE_D_SINGLE = (300, 2500, 6700)                       # single D blocks inside the DD runs of 256 and 1 024 blocks
_TILE_X = (7600, 7640)                                   # the extremes


def _tile_labels():
    lab = np.zeros(T, np.int8)
    for a, b in _TILE_DD:
        lab[a:b] = DD
    for a in _TILE_D_SINGLE:
        lab[a] = D
    lab[_TILE_X[0]:_TILE_X[1]] = X
    return lab


# PLAN_SMALL: 36 240 blocks = 289 921 samples (+ tail), 4.4 chain tiles, 35.4 three-launch tiles:
#   blocks 0 .. 1            DD from the stream's first block (d enters as 0)
#   blocks 2 .. 8 191        the tile motifs above
#   blocks 8 192 .. 33 467   ONE DD run of 3 x 8 192 + 700 = 25 276 blocks: it starts ON a chain-tile edge, the edges 16 384, 24 576 and 32 768
#                            lie inside it, tiles 1, 2 and 3 are a = 1 as a whole, m = 8 x count wraps 2^16 three times
#   block  33 468            a single D block, then DD again to 35 000 (a single D block inside a long DD stretch)
#   blocks 35 000 .. 36 239  D, with a single DD block at 35 500
SMALL_BLOCKS = 36240
LONG_RUN = (T, T + 3 * T + 700)


def _small_labels():
    lab = np.zeros(SMALL_BLOCKS, np.int8)
    lab[:T] = _tile_labels()
    lab[0:2] = DD
    lab[LONG_RUN[0]:LONG_RUN[1]] = DD
    lab[LONG_RUN[1] + 1:35000] = DD
    lab[35500] = DD
    return lab


PLAN_SMALL = plan_of_labels(_small_labels())
assert sum(k for _, k in PLAN_SMALL) == SMALL_BLOCKS and (DD, 25276) in PLAN_SMALL


def _many_labels(tiles):
    """the tile motifs in every tile; the tile edges t x 8 192 cycle through the four pairs -- t % 4 == 0: a DD run of 400 blocks across the
    edge (1,1); 1: a run that starts on it (0,1); 2: a run that ends on it (1,0); 3: D on both sides (0,0) -- and every 64th edge has
    (1,1) whatever t % 4 says (it is a multiple of 4); the run across every 512th edge starts 200 blocks before the tile in front of the edge,
    so that tile (511, 1 023, ...) is a = 1 as a whole with d entering, and so is tile 1 in front of edge 2, so that short streams have such
    a tile too.  (The tile BEHIND such an edge is not: the next edge's motif writes D over its last 200 blocks.)"""
    lab = np.tile(_tile_labels(), tiles)
    lab[0:2] = DD
    for t in range(1, tiles):
        e = t * T
        if t % 512 == 0 or t == 2:
            lab[max(0, e - T - 200):min(lab.size, e + T + 200)] = DD
        elif t % 4 == 0:
            lab[e - 200:e + 200] = DD
        elif t % 4 == 1:
            lab[e - 200:e] = D
            lab[e:e + 200] = DD
        elif t % 4 == 2:
            lab[e - 200:e] = DD
            lab[e:e + 200] = D
        else:
            lab[e - 200:e + 200] = D
    return lab


@lru_cache(maxsize=None)
def PLAN_MANY(tiles):
    """`tiles` chain tiles of 8 192 blocks: see _many_labels"""
    return plan_of_labels(_many_labels(int(tiles)))


@lru_cache(maxsize=None)
def plan_blocks(nblocks):
    """PLAN_MANY cut to exactly nblocks blocks"""
    nblocks = int(nblocks)
    return plan_of_labels(_many_labels(-(-nblocks // T))[:nblocks])


# ------------------------------------------------------------------------------------------------ dynamic delta: the input
def _fold(v):
    """reflect into [100, 500]: a walk with steps of at most 1 keeps steps of at most 1"""
    u = np.mod(v - 100, 800)
    return 100 + np.where(u <= 400, u, 800 - u)


def dyndelta_input(plan, seed, tail=0):
    """-> uint16 [1 + 8 x blocks + tail], read-only.  Vectorised over the whole stream (a plan of 4 M blocks takes a few seconds)."""
    assert 0 <= tail <= 7
    rng = np.random.default_rng(seed)
    choice = np.array([c for c, _ in plan], np.int8)
    nblk = np.array([k for _, k in plan], np.int64)
    keep = np.concatenate([[True], choice[1:] != choice[:-1]])                      # equal neighbours are one run
    rchoice = choice[keep]
    rlen = 8 * np.add.reduceat(nblk, np.flatnonzero(keep))                          # in samples
    rstart = np.concatenate([[0], np.cumsum(rlen)[:-1]])
    ns, nruns = int(rlen.sum()), rchoice.size
    assert rchoice[-1] != X and not ((rchoice[:-1] == X) & (rchoice[1:] != D)).any(), "a D segment must follow the extremes"
    kind = np.repeat(rchoice, rlen)
    idx = np.arange(ns, dtype=np.int32) - np.repeat(rstart, rlen).astype(np.int32)  # position inside the run
    diff = np.zeros(ns + tail, np.int32)

    # D: -, +, -, ... with magnitudes in [2 000, 3 000]
    mag = rng.integers(2000, 3001, size=ns, dtype=np.int32)
    np.copyto(diff[:ns], np.where(idx & 1, mag, -mag), where=kind == D)
    del mag
    # DD: the run's starting difference + the running sum of its second differences, reflected
    d0 = rng.integers(150, 451, size=nruns, dtype=np.int64)
    s = rng.integers(-1, 2, size=ns, dtype=np.int8)
    s[kind != DD] = 0
    if rchoice[0] == DD:
        s[0], s[1:8] = 0, 1            # the stream's first block: d enters as 0 and both errors of sample 0 are d0 -- a rising ramp makes
    cs = np.cumsum(s, dtype=np.int64)  # delta's loss the larger one under both losses
    cs -= np.repeat(cs[rstart] - s[rstart] - d0, rlen)
    np.copyto(diff[:ns], _fold(cs).astype(np.int32), where=kind == DD)
    del cs, s
    # the last difference of a D run in front of a DD run is that run's starting difference: the DD run is entered smoothly
    into = np.flatnonzero((rchoice[1:] == DD) & (rchoice[:-1] == D)) + 1
    diff[rstart[into] - 1] = d0[into]
    if tail:
        diff[ns:] = rng.integers(-3000, 3001, size=tail)
    x0 = int(rng.integers(0, 1 << 16))
    x = np.empty(ns + tail + 1, np.int64)
    x[0] = x0
    # run by run around the X runs (a handful): their samples are given, the differences resume from the last one (0)
    pos, cur = 0, x0
    vals = np.array([0, 0x8000, 0xffff], np.int64)
    for r in np.flatnonzero(rchoice == X):
        a, b = int(rstart[r]), int(rstart[r] + rlen[r])
        x[1 + pos:1 + a] = cur + np.cumsum(diff[pos:a], dtype=np.int64)
        i = np.arange(b - a)
        seg = np.where(i % 48 < 24, vals[i % 3], vals[rng.integers(0, 3, size=b - a)])   # the cycle, then drawn at random
        seg[-2:] = (0xffff, 0)
        x[1 + a:1 + b] = seg
        pos, cur = b, 0
    x[1 + pos:] = cur + np.cumsum(diff[pos:], dtype=np.int64)
    out = (x & 0xffff).astype(np.uint16)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=8)
def small_input(tail, seed=0):
    """PLAN_SMALL's stream with `tail` trailing elements (the golden set's inputs: seed 0)"""
    return dyndelta_input(PLAN_SMALL, seed + 100 * tail, tail)


def blocks_input(nblocks, seed, tail=0):
    return dyndelta_input(plan_blocks(nblocks), seed, tail)


# ------------------------------------------------------------------------------------------------ dynamic delta: reading a container
def choice_bits(container, n):
    """the (n - 1) // 8 choice bits of a dynamic-delta container of n elements (LSB first, behind the n elements)"""
    c = np.asarray(container, np.uint8)
    nblocks = max(n - 1, 0) // 8
    at = 4 + 2 * n
    return np.unpackbits(c[at:at + (nblocks + 7) // 8], bitorder="little")[:nblocks]


def run_lengths(bits):
    """-> (values, starts, lengths) of the runs of equal bits"""
    bits = np.asarray(bits)
    if bits.size == 0:
        return bits[:0], np.zeros(0, np.int64), np.zeros(0, np.int64)
    edges = np.flatnonzero(np.diff(bits)) + 1
    starts = np.concatenate([[0], edges])
    ends = np.concatenate([edges, [bits.size]])
    return bits[starts], starts, ends - starts


def _unzz(z):
    z = z.astype(np.int64)
    return (z >> 1) ^ -(z & 1)


def dyndelta_model(container, n):
    """decoder from the format: element 0 verbatim; per block of 8, zigzagged errors of the chosen predictor -- delta: x += e; double delta:
    d += e, x += d, d being the last TRUE difference whichever predictor coded it; the < 8 trailing elements are plain delta errors.  One
    run of equal choices at a time: cumulative sums in int64 (a run of 300 K samples of |e| < 2^15 stays below 2^51), reduced mod 2^16 at
    the run's end."""
    c = np.asarray(container, np.uint8)
    assert int(c[:4].view(np.uint32)[0]) == n
    if n == 0:
        return np.zeros(0, np.uint16)
    w = c[4:4 + 2 * n].view(np.uint16)
    out = np.empty(n, np.uint16)
    out[0] = w[0]
    x, d = int(w[0]), 0
    bits = choice_bits(c, n)
    vals, starts, lens = run_lengths(bits)
    for v, a, k in zip(vals, starts, lens):
        e = _unzz(w[1 + 8 * a:1 + 8 * (a + k)])
        if v:
            dd = d + np.cumsum(e)
            xx = x + np.cumsum(dd)
            d = int(dd[-1]) & 0xffff
        else:
            xx = x + np.cumsum(e)
            d = int(e[-1]) & 0xffff
        x = int(xx[-1]) & 0xffff
        out[1 + 8 * a:1 + 8 * (a + k)] = xx & 0xffff
        if d >= 0x8000:
            d -= 0x10000                                    # (any representative of d mod 2^16 gives the same samples)
    nb = bits.size
    tail = w[1 + 8 * nb:n].astype(np.int64)
    out[1 + 8 * nb:] = (x + np.cumsum(tail)) & 0xffff
    return out


def dyndelta_model_slow(container, n):
    """the same, one Python-int pass (for short streams: a check on the check)"""
    c = np.asarray(container, np.uint8)
    w = [int(v) for v in c[4:4 + 2 * n].view(np.uint16)]
    bits = choice_bits(c, n)
    out = [w[0]]
    x, d = w[0], 0
    for b in range(bits.size):
        for i in range(8):
            z = w[1 + 8 * b + i]
            e = (z >> 1) ^ -(z & 1)
            d = (d + e if bits[b] else e) & 0xffff
            x = (x + d) & 0xffff
            out.append(x)
    for at in range(1 + 8 * bits.size, n):
        x = (x + w[at]) & 0xffff
        out.append(x)
    return np.array(out, np.uint16)


# ------------------------------------------------------------------------------------------------ coverage, read from a container
def longest_dd_run(bits):
    vals, _, lens = run_lengths(bits)
    return int(lens[vals == 1].max()) if (vals == 1).any() else 0


def pairs_at(bits, B):
    """the set of (choice before, choice after) over the multiples of B"""
    at = np.arange(B, bits.size, B)
    return {(int(a), int(b)) for a, b in zip(bits[at - 1], bits[at])}


def whole_dd_tiles_with_d(container, n):
    """chain tiles that are a = 1 as a whole (every block double delta) with d != 0 entering: the difference of the two samples in front"""
    bits = choice_bits(container, n)
    x = dyndelta_model(container, n)
    hits = []
    for t in range(1, bits.size // T):
        if bits[t * T:(t + 1) * T].all() and x[8 * t * T] != x[8 * t * T - 1]:
            hits.append(t)
    return hits


def has_zigzag_ffff(container, n):
    nb = max(n - 1, 0) // 8
    return bool((np.asarray(container, np.uint8)[6:6 + 16 * nb].view(np.uint16) == 0xffff).any())


# ------------------------------------------------------------------------------------------------ sprintzpack
PACK_STRIDE = 2048             # a width's stretch starts every 2 048 blocks (on a tile edge) and is PACK_STRETCH long; the rest changes width every block
PACK_STRETCH = 1030
PACK_PERIOD = 17 * PACK_STRIDE
PACK_SMALL_BLOCKS = SMALL_BLOCKS


def pack_widths(seed, nblocks):
    """the bit length of every block's OR: per period of 34 816 blocks, for w = 0 .. 16 a stretch of 1 030 blocks of width w from block
    2 048 w on (a whole 1 024-block tile and 6 blocks of the next), then 1 018 blocks whose width changes every block -- the first 256 of
    them alternating escape blocks (16 and 15: nibble 15, 16 bytes) with widths 0, 1 and 2, the others drawn from 0 .. 16"""
    rng = np.random.default_rng(seed)
    b = np.arange(nblocks, dtype=np.int64)
    p = b % PACK_PERIOD
    w = p // PACK_STRIDE
    o = p % PACK_STRIDE
    mixed = np.cumsum(rng.integers(1, 17, size=nblocks)) % 17                        # never the same width twice in a row
    alt = np.where(o & 1, (o >> 1) % 3, 16 - ((o >> 1) & 1))
    return np.where(o < PACK_STRETCH, w, np.where(o < PACK_STRETCH + 256, alt, mixed)).astype(np.int64)


def pack_input(seed, nblocks, zig=False, tail=0):
    """-> uint16 [8 x nblocks + tail], read-only: blocks whose values' OR (kind 3) or whose zigzagged values' OR (zig: kind 4) has exactly
    pack_widths' bit length"""
    rng = np.random.default_rng(seed + 1)
    w = pack_widths(seed, nblocks)
    v = rng.integers(0, 1 << 16, size=(nblocks, 8), dtype=np.int64)
    v &= ((1 << w) - 1)[:, None]
    v[:, 0] |= np.where(w > 0, 1 << np.maximum(w - 1, 0), 0)
    v = v.ravel()
    if zig:
        v = ((v >> 1) ^ -(v & 1)) & 0xffff
    out = np.concatenate([v, rng.integers(0, 1 << 16, size=tail, dtype=np.int64)]).astype(np.uint16)
    out.setflags(write=False)
    return out


def pack_nibbles(container, n):
    """the n // 8 header nibbles of a sprintzpack container of n values"""
    c = np.asarray(container, np.uint8)
    nblocks = n // 8
    hb = c[4:4 + (nblocks + 1) // 2]
    return np.stack([hb & 15, hb >> 4], axis=1).ravel()[:nblocks]


def tile_payloads(nibbles):
    """payload bytes of every whole 1 024-block tile (nibble 15 means 16 bytes)"""
    nb = np.asarray(nibbles, np.int64)
    nb = nb + (nb == 15)
    k = nb.size // 1024
    return nb[:k * 1024].reshape(k, 1024).sum(axis=1)


def nibbles_owning_a_tile(nibbles):
    """the nibble values that fill at least one aligned 1 024-block tile"""
    nb = np.asarray(nibbles)
    k = nb.size // 1024
    t = nb[:k * 1024].reshape(k, 1024)
    same = (t == t[:, :1]).all(axis=1)
    return {int(v) for v in t[same, 0]}


# ------------------------------------------------------------------------------------------------ against the compiled reference
def ref_pack(ref, kind, x):
    """ref: oracle/_ref's library, loaded.  -> (the container its *_pack_u16 writes, bytes it leaves unwritten as 0; the mask of the bytes it
    writes, found by running it over two differently filled buffers; its return value).  Its own decoder must restore x.  Shared by the tests
    and by the recipe that mints the golden set (oracle/gen_golden_online_drive.py)"""
    import ctypes as C
    ref.ref_online_pack.restype = C.c_int64
    ref.ref_online_pack.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    ref.ref_online_unpack.restype = C.c_int64
    ref.ref_online_unpack.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    x = np.ascontiguousarray(x, dtype=np.uint16)
    n = x.size
    cap = 2 * n + n // 8 + 256
    a, b = np.zeros(cap, np.uint8), np.full(cap, 0xFF, np.uint8)
    ra = ref.ref_online_pack(kind, x.ctypes.data, n, a.ctypes.data)
    rb = ref.ref_online_pack(kind, x.ctypes.data, n, b.ctypes.data)
    assert ra == rb, (kind, n)
    nbytes = 2 * int(ra)
    back = np.zeros(n + 16, np.uint16)
    assert ref.ref_online_unpack(kind, a.ctypes.data, back.ctypes.data) == n and np.array_equal(back[:n], x), (kind, n)
    return a[:nbytes].copy(), a[:nbytes] == b[:nbytes], int(ra)


def reference_agrees(ref, kind, x, got, ret):
    """got, ret: a container of x and its return value (the oracle's).  The compiled reference returns the same value and writes the same
    bytes -- those it writes at all; `got` has 0 in the others -- and its decoder restores the input (ref_pack)"""
    cont, defined, rret = ref_pack(ref, kind, x)
    assert ret == rret and got.size == cont.size, (kind, x.size)
    assert np.array_equal(got[defined], cont[defined]) and not got[~defined].any(), (kind, x.size)


# ------------------------------------------------------------------------------------------------ the golden set (oracle/gen_golden_online_drive.py)
GOLDEN_SEED = 0
GOLDEN_STORED_TAIL = 5                                   # the one PLAN_SMALL container stored whole (kinds 0 and 1); the others: length, return value, CRC32


def golden_cases():
    """-> [(name, kind, input)]: PLAN_SMALL with every tail under both losses, the pack input at the same size under kinds 3 and 4"""
    cases = []
    for kind in (0, 1):
        for tail in range(8):
            cases.append((f"small_k{kind}_t{tail}", kind, small_input(tail, GOLDEN_SEED)))
    for kind in (3, 4):
        cases.append((f"pack_k{kind}", kind, pack_input(GOLDEN_SEED, PACK_SMALL_BLOCKS, zig=kind == 4, tail=3)))
    return cases
