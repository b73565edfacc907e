"""Inputs that STEER the RLE / group state machine of the codec -- which slot of a group a run closes in, a
packed block that becomes slot 0 of a new group, the `<=` / `<` tail test, the 0x00 padding slot, the 1- and 2-byte run length, the
cap of 32 767 blocks -- where every other input of the suite leaves the runs to a random walk with flat spans on multiples of 8 blocks.

Plain numpy; nothing here is product code or oracle code.  Four pieces:

  schedule     which blocks of a chunk are all-zero: segments of [g packed blocks][L zero blocks], g cycling 1, 2, 3, behind a prefix
               that depends on the chunk's index, so that over 16 chunks every run edge sits on 16 consecutive block indices
  samples      rows that have exactly those all-zero blocks, for the delta codecs and (through tests/fire_drive.py) for FIRE
  slots        a parser of the stream's framing (A.1 / A.2 / A.4): the (group, slot, kind, length) of every slot
  model_slots  an independent restatement of A.5 on the all-zero flags: the slots an encoder must write

Expected bytes are always the oracle's; the parser and the model are for coverage assertions and for saying WHICH rule a stream broke."""
from functools import lru_cache

import numpy as np

import fire_drive as fd
from harness import DTYPES

KINDS = ("lengths", "varint", "alternate", "start", "tails")
CAP = 32767                    # blocks a run slot can stand for (sprintz_xff_rle.cpp:71)
G = (1, 2, 3)                  # packed blocks in front of each run, in turn: runs close in both slots of a group


def _segments(out, pos, lengths, k0=0, stop=None):
    """[g packed][L zero] segments from block pos on, L from `lengths` in turn, while a whole segment and a packed block behind it fit
    before `stop`; out[] starts all-packed.  -> the first block behind the last run"""
    stop = out.size if stop is None else stop
    k = k0
    while True:
        g, L = G[k % 3], lengths[k % len(lengths)]
        if pos + g + L + 1 > stop:
            return pos
        out[pos + g:pos + g + L] = True
        pos += g + L
        k += 1


def schedule(kind, nblocks, rot):
    """-> bool[nblocks]: True = the block is all-zero.  rot is the chunk's index in its batch"""
    z = np.zeros(nblocks, bool)
    p = rot % 16
    if kind == "lengths":                        # L = 1 .. 16 in turn; a short chunk starts the turn where its pair of rotations says
        first = ((rot >> 1) * 5) % 16
        _segments(z, p, [1 + (first + j) % 16 for j in range(16)])
    elif kind == "varint":                       # 126 .. 129: both sides of the second length byte; one run a chunk, two where they fit
        pos = p
        for j, L in enumerate((126 + (rot >> 1) % 4, 126 + (rot >> 3) % 4)):
            g = G[j]
            if j and pos + g + L + 3 > nblocks:
                break
            z[pos + g:pos + g + L] = True        # (a chunk too short for the run: it is cut at the chunk's end)
            pos += g + L
    elif kind == "alternate":                    # zero / packed / zero / ...: every run is one block, every group rolls over
        z[p::2] = True
    elif kind == "start":                        # block 0 is zero: L = 1 (rot = 0, 16, ...) and L > 1; the stream's first slot is a run
        L0 = min(1 + p, nblocks - 3)
        z[:L0] = True
        _segments(z, L0, list(range(2, 12)), k0=rot)
    elif kind == "tails":                        # ... [run Lf][k packed] at the chunk's end; k = 0: the run reaches the end
        k, Lf = rot % 4, (1, 2, 3, 5)[(rot >> 2) % 4]
        front = nblocks - k - Lf
        _segments(z, p, [1, 2, 3, 4, 5], k0=rot >> 1, stop=front)
        # the slots in front (a packed block each, a run each) put the final run in slot (rot >> 2) & 1: where they do not, the last
        # run of two blocks or more gives its first block to the packed ones
        starts = np.flatnonzero(z[:front] & ~np.concatenate([[False], z[:front - 1]]))
        if (int((~z[:front]).sum()) + starts.size) % 2 != (rot >> 2) & 1:
            long = [s for s in starts if z[s + 1]]
            if long:
                z[long[-1]] = False
        z[front:front + Lf] = True
    else:
        raise ValueError(kind)
    return z


def schedules(kind, nchunks, nblocks):
    return np.stack([schedule(kind, nblocks, c) for c in range(nchunks)])


@lru_cache(maxsize=None)
def _fire_base(w, lowdim, key, shape, seed):
    """FIRE trajectories of `gen` columns a chunk, the chunks side by side as columns of one fire_drive.drive call: a run block has
    delta = pred under whatever coefficient is frozen"""
    zero = np.frombuffer(key, bool).reshape(shape)
    nchunks, nblocks = shape
    gen = (4 if w == 8 else 2) if lowdim else fd.TILE
    dirs = np.concatenate([fd.directions(gen, (2, 3, 0, 1, 4, 5, 6)[c % 7]) for c in range(nchunks)])
    x = fd.drive(w, lowdim, dirs, seed, nblocks, runs=np.repeat(zero.T, gen, axis=1))[0]
    x = np.ascontiguousarray(x.reshape(8 * nblocks, nchunks, gen).transpose(1, 0, 2))
    x.setflags(write=False)
    return x


def samples(codec, w, D, zero_blocks, seed=0):
    """zero_blocks: bool[nchunks, nblocks] -> samples [nchunks, 8 * nblocks, D] whose all-zero blocks (errors of `codec`) are exactly those.
    delta: a zero block repeats the previous row; a packed block steps every column by -1 / 0 / +1 times an amplitude of the COLUMN's own
    (0, 1, 2, 4 .. 2^(w-1): every width in one row, rows that end inside a byte), column 0 always moving in the block's first row.
    xff: tests/fire_drive.py's forecaster, one schedule a chunk"""
    zero_blocks = np.asarray(zero_blocks, bool)
    nchunks, nblocks = zero_blocks.shape
    if codec == "xff":
        lowdim = fd.is_lowdim(w, D)
        base = _fire_base(w, lowdim, zero_blocks.tobytes(), zero_blocks.shape, seed)
        gen = base.shape[2]
        return np.tile(base, (1, 1, -(-D // gen)))[:, :, :D] if D > gen else base[:, :, :D]
    assert codec == "delta"
    rng = np.random.default_rng(seed)
    amp = (1 << rng.integers(0, w + 1, (nchunks, 1, D))) >> 1
    amp[:, :, 0] = np.maximum(amp[:, :, 0], 1)
    steps = rng.integers(-1, 2, (nchunks, 8 * nblocks, D)) * amp
    steps[:, ::8, 0] = amp[:, :, 0]
    steps[np.repeat(zero_blocks, 8, axis=1)] = 0
    return (np.cumsum(steps, axis=1) & ((1 << w) - 1)).astype(DTYPES[w // 8])


def batch(codec, w, D, kind, nchunks, nblocks, r=0, seed=0):
    """-> (flat samples, chunk_len, zero_blocks): nchunks chunks of nblocks blocks and r more elements (r > 0: chunk lengths that are no
    whole blocks, where `<=` and `<` stop alike), the chunk c on schedule(kind, nblocks, c)"""
    zero = schedules(kind, nchunks, nblocks)
    x = samples(codec, w, D, zero, seed).reshape(nchunks, -1)
    if r:
        tail = np.random.default_rng(seed + 77).integers(0, 1 << w, (nchunks, r)).astype(x.dtype)
        x = np.concatenate([x, tail], axis=1)
    return np.ascontiguousarray(x).ravel(), 8 * nblocks * D + r, zero


def cap_chunks(codec, w, D, nchunks=3, nzero=70000, seed=0):
    """nchunks chunks of nzero all-zero blocks and two packed ones: runs of 32 767, 32 767 and the rest -> (flat samples, chunk_len, zero_blocks)"""
    zero = np.zeros((nchunks, nzero + 2), bool)
    zero[:, :nzero] = True
    tail = samples(codec, w, D, np.zeros((nchunks, 2), bool), seed)          # (zero samples are zero errors under either codec, from a zero state)
    x = np.zeros((nchunks, 8 * (nzero + 2), D), tail.dtype)
    x[:, 8 * nzero:] = tail
    return x.ravel(), 8 * (nzero + 2) * D, zero


def is_lowdim(w, D):
    return D <= (4 if w == 8 else 2)


def slots(stream, w, D):
    """parse a stream's framing (A.1, A.2 / A.4) -> (ngroups, remaining_len, [(group, slot, "run" | "block" | "pad", length)]); length is in
    blocks (1 for a packed block, 0 for the padding slot).  Raises if the groups and the verbatim tail are not exactly the stream"""
    s = np.asarray(stream, np.uint8)
    esz, hb = w // 8, 3 if w == 8 else 4
    ngroups = int(s[0]) | int(s[1]) << 8 | int(s[2]) << 16 | int(s[3]) << 24
    remaining = int(s[4]) | int(s[5]) << 8
    assert (int(s[6]) | int(s[7]) << 8) == D, "ndims"
    hbytes = (2 * D * hb + 7) // 8
    lowdim = is_lowdim(w, D)
    pos, out = 8, []
    for g in range(ngroups):
        bits = np.unpackbits(s[pos:pos + hbytes], bitorder="little")[:2 * D * hb].reshape(2, D, hb)
        fields = (bits * (1 << np.arange(hb))).sum(axis=2)
        pos += hbytes
        for b in range(2):
            if not fields[b].any():
                n = int(s[pos]) & 0x7f
                if s[pos] & 0x80:
                    n |= int(s[pos + 1]) << 7
                    pos += 1
                pos += 1
                out.append((g, b, "run" if n else "pad", n))
            else:
                nbits = np.where(fields[b] == w - 1, w, fields[b])
                pos += int(nbits.sum()) if lowdim else 8 * ((int(nbits.sum()) + 7) // 8)
                out.append((g, b, "block", 1))
    if pos + remaining * esz != s.size:
        raise AssertionError(f"framing: {ngroups} groups end at byte {pos}, {remaining} verbatim elements, stream of {s.size} bytes")
    return ngroups, remaining, out


def model_slots(zero_blocks, n, D, blk=8, tail_le=False):
    """A.5 on the all-zero flags of a chunk of n elements (blocks of blk rows): -> (ngroups, remaining_len, the list `slots` returns).
    tail_le: the general FIRE codec's `<=` in the test behind a run block (sprintz_xff_rle.cpp:362); every other codec tests `<`"""
    be = blk * D

    def fits(i):                                 # the outer guard: two more blocks
        return (i + 2) * be <= n

    def goes_on(i):                              # the test behind a run block
        return (i + 2) * be <= n if tail_le else (i + 2) * be < n

    out, i, run, g, done = [], 0, 0, -1, False
    while not done and fits(i):
        g, b = g + 1, 0
        while b < 2 and not done:
            z = bool(zero_blocks[i])
            rle = z and run < CAP
            while True:
                if rle:
                    run, i = run + 1, i + 1
                    if goes_on(i):
                        break                    # the next block, the same slot
                    out.append((g, b, "run", run))
                    out.extend((g, s, "pad", 0) for s in range(b + 1, 2))
                    run, done = 0, True
                    break
                if run > 0:                      # a packed block, or the cap, closes the run
                    out.append((g, b, "run", run))
                    b, run = b + 1, 0
                    if b == 2:                   # ... and the block at hand becomes slot 0 of a new group
                        g, b = g + 1, 0
                    if z:
                        rle = True
                        continue
                out.append((g, b, "block", 1))
                i, b = i + 1, b + 1
                break
    return g + 1, n - i * be, out
