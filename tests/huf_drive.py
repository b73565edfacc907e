"""The Huffman drive: inputs that steer the shared code-table builder (huf_build_kernel, sprintz_amd/csrc/huf.hip) and the container
writer / reader behind it through the paths that Sprintz streams of natural data do not reach, plus two independent opinions.

  lengths_model(counts)      a plain restatement of the code-length specification in the header of oracle/huf_oracle.c that also reports
                             WHICH paths ran (depth, clamp, repair rounds, the quarter of the sorted leaves a round moved, ties)
  decode_record(record, t)   a bit reader of one record of our container that shares no code with the model or with the oracle
  HISTOGRAMS                 named 256-entry count vectors (degenerate, deep, the 64 / 128 / 192-leaf ladder, long repairs, ties)
  segment(counts, sizes, ..) a histogram laid out as chunks that hold exactly those counts
  RECORD_CASES               chunks, inside suitable segments, whose records sit on both sides of every edge of the container
  BATCHES                    all of it as seven containers: 1 / 63 / 64 / 65 / 129 / 769 / 833 chunks, 16-byte aligned and byte-dense from an
                             odd address, three of them ending 0 / 4 / 60 bytes into a 64-byte line
  (the three tables are built on first use: histograms(), edge_segments(), batches())

No GPU and no oracle in here: tests/test_huf_drive_cpu.py proves that every input gets where it claims to, tests/test_gpu_huf_drive.py
runs the kernels on them.  Everything is exact (tables, bytes, offsets)."""
from functools import lru_cache

import numpy as np

LMAX = 11
SEG = 64


# ----------------------------------------------------------------- opinion 1: the code lengths, with the paths they took

def lengths_model(counts, lengthen_tie="largest", shorten_tie="smallest", equal_weight="leaf"):
    """-> (lens uint8[256], stats).  The keyword arguments select the specification (the defaults) or one of its mutants:
    lengthen_tie="smallest", shorten_tie="largest", equal_weight="internal"."""
    counts = [int(c) for c in counts]
    assert len(counts) == 256 and min(counts) >= 0
    lens = np.zeros(256, np.uint8)
    leaves = sorted((c, s) for s, c in enumerate(counts) if c)                  # lower count first, then lower symbol
    nz = len(leaves)
    stats = dict(nz=nz, depth=0, clamped=0, kraft=0, up=0, down=0, up_quarters=[], down_quarters=[], up_symbol_ties=0,
                 down_symbol_ties=0, merge_ties=[0, 0])
    if nz == 0:
        return lens, stats
    if nz == 1:
        lens[leaves[0][1]] = 1
        stats.update(depth=1, kraft=1 << (LMAX - 1))
        return lens, stats
    # two queues: the sorted leaves, and the internal nodes in the order they were made
    weight = [c for c, _ in leaves]
    parent = {}
    ql, qi = 0, nz
    for _ in range(nz - 1):
        pair = []
        for pick in range(2):
            leaf_ok, internal_ok = ql < nz, qi < len(weight)
            if leaf_ok and internal_ok and weight[ql] == weight[qi]:
                stats["merge_ties"][pick] += 1
                take_leaf = equal_weight == "leaf"
            else:
                take_leaf = leaf_ok and (not internal_ok or weight[ql] < weight[qi])
            if take_leaf:
                pair.append(ql)
                ql += 1
            else:
                pair.append(qi)
                qi += 1
        parent[pair[0]] = parent[pair[1]] = len(weight)
        weight.append(weight[pair[0]] + weight[pair[1]])
    root = len(weight) - 1
    depth = []
    for i in range(nz):
        d, node = 0, i
        while node != root:
            node, d = parent[node], d + 1
        depth.append(d)
    ln = [min(d, LMAX) for d in depth]
    full = 1 << LMAX
    kraft = sum(full >> l for l in ln)
    stats.update(depth=max(depth), clamped=sum(d > LMAX for d in depth), kraft=kraft)
    # too many codes: lengthen the deepest code below LMAX; ties to the smallest count, then the largest symbol
    while kraft > full:
        cand = [i for i in range(nz) if ln[i] < LMAX]
        deepest = max(ln[i] for i in cand)
        cand = [i for i in cand if ln[i] == deepest]
        least = min(leaves[i][0] for i in cand)
        cand = [i for i in cand if leaves[i][0] == least]
        stats["up_symbol_ties"] += len(cand) > 1
        i = max(cand, key=lambda k: leaves[k][1]) if lengthen_tie == "largest" else min(cand, key=lambda k: leaves[k][1])
        kraft -= full >> (ln[i] + 1)
        ln[i] += 1
        stats["up"] += 1
        stats["up_quarters"].append(i // 64)
    # room left: shorten the most frequent symbol whose shorter code still fits; ties to the smallest symbol
    while True:
        cand = [i for i in range(nz) if ln[i] > 1 and kraft + (full >> ln[i]) <= full]
        if not cand:
            break
        most = max(leaves[i][0] for i in cand)
        cand = [i for i in cand if leaves[i][0] == most]
        i = min(cand, key=lambda k: leaves[k][1]) if shorten_tie == "smallest" else max(cand, key=lambda k: leaves[k][1])
        stats["down_symbol_ties"] += any(k != i and ln[k] == ln[i] for k in cand)
        kraft += full >> ln[i]
        ln[i] -= 1
        stats["down"] += 1
        stats["down_quarters"].append(i // 64)
    for i, (_, s) in enumerate(leaves):
        lens[s] = ln[i]
    return lens, stats


MUTANTS = {
    "lengthening ties to the smallest symbol": dict(lengthen_tie="smallest"),
    "shortening ties to the largest symbol": dict(shorten_tie="largest"),
    "internal node before leaf on equal weight": dict(equal_weight="internal"),
}


# ----------------------------------------------------------------- opinion 2: one record of the container, read bit by bit

def record_header(record):
    """-> (n, stored, [sz0, sz1, sz2] or None) of the record that starts at record[0]"""
    hdr = int.from_bytes(bytes(record[:4]), "little")
    n, stored = hdr & 0x7FFFFFFF, bool(hdr >> 31)
    if stored:
        return n, True, None
    return n, False, [int.from_bytes(bytes(record[4 + 2 * k:6 + 2 * k]), "little") for k in range(3)]


def decode_record(record, table_nibbles, per_stream=None):
    """One record (its bytes up to the next record's start; trailing padding allowed) with its segment's 128-byte nibble table ->
    the chunk's bytes.  per_stream=K decodes only the first K symbols of each of the four sub-streams and returns (bytes, mask of
    the positions decoded): every sub-stream's start depends on the header's sizes, which is what a long edge record is about."""
    record = bytes(record)
    n, stored, sz = record_header(record)
    out = bytearray(n)
    mask = np.zeros(n, bool)
    if stored:
        out[:] = record[4:4 + n]
        mask[:] = True
        return bytes(out) if per_stream is None else (bytes(out), mask)
    # canonical code of every symbol: by length, then by symbol value; written into the stream from its TOP bit down, so the
    # reader below, which takes the stream's bits in order (byte by byte, least significant first), sees a code top bit first
    length = {}
    for s in range(256):
        nib = table_nibbles[s >> 1]
        l = int(nib) >> 4 if s & 1 else int(nib) & 15
        if l:
            length[s] = l
    book, code, prev = {}, 0, 0
    for s, l in sorted(length.items(), key=lambda kv: (kv[1], kv[0])):
        code <<= l - prev
        book[(l, code)] = s
        code, prev = code + 1, l
    assert record[10:12] == b"\0\0"
    q = (n + 3) // 4
    start = 12
    for j in range(4):
        a, b = min(j * q, n), min(j * q + q, n)
        if per_stream is not None:
            b = min(b, a + per_stream)
        pos, bit = start, 0
        for i in range(a, b):
            l, code = 0, 0
            while True:
                code = (code << 1) | ((record[pos] >> bit) & 1)
                l += 1
                bit += 1
                if bit == 8:
                    pos, bit = pos + 1, 0
                if (l, code) in book:
                    break
                assert l < LMAX, ("no code of the table matches", j, i)
            out[i] = book[(l, code)]
            mask[i] = True
        if j < 3:
            start += sz[j]
    return bytes(out) if per_stream is None else (bytes(out), mask)


# ----------------------------------------------------------------- histograms

def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def _place(values, where="low"):
    """a list of counts on symbol values: 'low' 0.., 'high' ..255, 'spread' evenly over 0..255 (absent symbols interleaved)"""
    h = np.zeros(256, np.int64)
    k = len(values)
    if where == "low":
        idx = np.arange(k)
    elif where == "high":
        idx = np.arange(256 - k, 256)
    else:
        idx = (np.arange(k) * 256) // k
    h[idx] = values
    return h


def _ladder(nz, where):
    """a deep histogram of nz symbols within ~0.32 MB: Fibonacci counts under the cap, equal counts at it"""
    f = _fib(24)
    vals = [1 + (i % 3) for i in range(nz - 24)] + f
    return _place(vals[:nz] if nz >= 24 else f[:nz], where)


def _shorten_search():
    """a seeded search: log-normal counts on 60 .. 255 symbols, the draw of 400 with the most shortening rounds within a 0.5 MB total"""
    rng = np.random.default_rng(2024)
    best, best_h = -1, None
    for _ in range(400):
        k = int(rng.integers(60, 256))
        c = np.exp(rng.normal(0.0, rng.uniform(2.0, 4.5), k))
        c = np.maximum(1, c * (400000.0 / c.sum())).astype(np.int64)
        h = np.zeros(256, np.int64)
        h[rng.permutation(256)[:k]] = c
        if h.sum() > 500000:
            continue
        down = lengths_model(h)[1]["down"]
        if down > best:
            best, best_h = down, h
    return best_h


@lru_cache(maxsize=None)
def histograms():
    """name -> int64[256]; insertion order is the drive's order"""
    H = {}
    H["no symbol"] = _place([])
    H["one symbol"] = np.roll(_place([5000]), 77)
    H["two symbols"] = np.roll(_place([4000, 9], "low"), 200)
    H["three equal"] = _place([700, 700, 700], "spread")
    H["depth 11"] = _place([int(1.8 ** i) + 1 for i in range(12)], "low")
    H["depth 12"] = _place([int(1.8 ** i) + 1 for i in range(13)], "spread")
    H["fib 24 low"] = _place(_fib(24), "low")
    H["fib 24 high"] = _place(_fib(24), "high")
    for k, nz in enumerate((63, 64, 65, 128, 129, 192, 193, 255, 256)):
        where = ("low", "high", "spread")[k % 3]
        H["ladder %d %s" % (nz, where)] = _ladder(nz, where)
    H["fib 30 + 226 ones"] = _place([1] * 226 + _fib(30), "low")
    H["powers + 244 ones"] = _place([1] * 244 + [1 << k for k in range(7, 19)], "high")
    H["shorten search"] = _shorten_search()
    H["ties up"] = _place([1 + i // 2 for i in range(256)], "low")
    H["ties up, levels"] = _levels(256, 1.35, 8)
    H["ties down"] = _levels(241, 1.273, 6)
    H["all equal"] = _place([300] * 256)
    H["all ones"] = _place([1] * 256)
    for h in H.values():
        h.setflags(write=False)
    return H


def _levels(k, ratio, per):
    """k symbols, `per` of them on each geometric level: many leaves equal in count and, after the clamp, in length"""
    vals = []
    for level in range((k + per - 1) // per):
        vals += [int(ratio ** level) + 1] * per
    return _place(vals[:k], "low")


# ----------------------------------------------------------------- segments: 64 chunks that hold exactly a histogram

def _rng(name):
    import zlib
    return np.random.default_rng(zlib.crc32(name.encode()))


def _cuts(total, parts, rng):
    """`parts` sizes that sum to `total`, a few of them 0"""
    if parts == 1:
        return [int(total)]
    cuts = np.sort(rng.integers(0, total + 1, parts - 1))
    return np.diff(np.concatenate([[0], cuts, [total]])).astype(np.int64).tolist()


def segment(counts, sizes, rng, fixed=None):
    """counts laid out as len(sizes) chunks of those sizes (-1: whatever is left over, shared out at random among the -1 entries).
    fixed: {chunk index: bytes} are taken as they are, and their symbols come out of `counts`."""
    fixed = fixed or {}
    left = np.array(counts, np.int64)
    for ch in fixed.values():
        left -= np.bincount(ch, minlength=256)
    assert (left >= 0).all(), "the fixed chunks hold more of a symbol than the histogram"
    pool = np.repeat(np.arange(256, dtype=np.uint8), left)
    rng.shuffle(pool)
    sizes = list(sizes)
    free = [k for k, s in enumerate(sizes) if s < 0 and k not in fixed]
    known = sum(s for k, s in enumerate(sizes) if s >= 0 and k not in fixed)
    assert known <= pool.size and (free or known == pool.size), (known, pool.size)
    for k, s in zip(free, _cuts(pool.size - known, len(free), rng) if free else []):
        sizes[k] = s
    chunks, at = [], 0
    for k, s in enumerate(sizes):
        if k in fixed:
            chunks.append(np.asarray(fixed[k], np.uint8))
        else:
            chunks.append(pool[at:at + s].copy())
            at += s
    assert at == pool.size
    return chunks


def record_sizes(chunk, lens):
    """the drive's own size arithmetic (numpy): -> (stored, [sz0 .. sz3]) of a chunk under a length table"""
    n = len(chunk)
    q = (n + 3) // 4
    bits = np.asarray(lens, np.int64)[np.asarray(chunk, np.uint8)]
    sz = [int(-(-int(bits[min(j * q, n):min(j * q + q, n)].sum()) // 8)) for j in range(4)]
    stored = 12 + sum(sz) >= 4 + n or max(sz[:3]) > 0xFFFF
    return stored, sz


GEO = [1 << (LMAX - 1 - k) for k in range(LMAX)] + [1]         # 12 symbols: lengths 1, 2, .. 10, 11, 11 (symbol k: k + 1 bits)
SMALL_SIZES = list(range(18)) + [4095, 4096, 4097, 8192 + 5]  # 256 16-byte pieces are one trip of a workgroup in K1 and K2


def _geo_counts(scale, base=0):
    h = np.zeros(256, np.int64)
    h[base:base + 12] = np.array(GEO) * scale
    return h


def _with_lengths(n, per_stream_short, long_sym, short_sym):
    """n = 4q symbols of `long_sym`, the first per_stream_short[j] of sub-stream j replaced by `short_sym`"""
    q = n // 4
    ch = np.full(n, long_sym, np.uint8)
    for j, k in enumerate(per_stream_short):
        ch[j * q:j * q + k] = short_sym
    return ch


@lru_cache(maxsize=None)
def edge_segments():
    """-> ({segment name: chunks}, [record cases]).  A case: dict(segment, chunk, what, stored, and where it applies sub = (j, bytes)
    or enc_minus_n) -- the side of the edge the record must be on, which the tests read back from the record's header."""
    segs, cases = {}, []

    # stored rule 12 + enc >= 4 + n, and the chunk sizes around a workgroup's trip.  Symbol 7 costs 8 bits, symbol 6 costs 7: 128
    # symbols of 8 bits are enc == n; 24 seven-bit symbols in a sub-stream take 3 bytes off, 16 take 2.
    name = "edge: stored rule, sizes"
    base = 40
    fixed = {20: _with_lengths(128, (24, 24, 24, 0), base + 7, base + 6),        # enc == n - 9: coded
             21: _with_lengths(128, (24, 24, 16, 0), base + 7, base + 6)}        # enc == n - 8: stored
    sizes = SMALL_SIZES[:18] + [-1, -1, 128, 128] + SMALL_SIZES[18:] + [-1] * 38
    segs[name] = segment(_geo_counts(48, base), sizes, _rng(name), fixed)
    cases.append(dict(segment=name, chunk=20, what="enc == n - 9", stored=False, enc_minus_n=-9))
    cases.append(dict(segment=name, chunk=21, what="enc == n - 8", stored=True, enc_minus_n=-8))
    for k, s in enumerate(sizes):
        if s in SMALL_SIZES and k not in fixed:
            cases.append(dict(segment=name, chunk=k, what="size %d" % s, n=s))

    # the 16-bit size fields: symbol 0 costs 1 bit, symbols 100 .. 115 cost 5.  104 856 five-bit symbols are exactly 65 535 bytes,
    # 104 857 are 65 536.  Sub-streams 0 .. 2 have a size field (one byte too many: stored); the fourth has none and stays coded.
    name = "edge: 16-bit sizes, one sub-stream"
    fixed = {}
    for j in range(4):
        for k, q in enumerate((104856, 104857)):
            ch = np.zeros(4 * q, np.uint8)
            ch[j * q:(j + 1) * q] = 100 + (np.arange(q) * 7 + j) % 16
            at = 3 + 7 * (2 * j + k)
            fixed[at] = ch
            over = k == 1
            cases.append(dict(segment=name, chunk=at, what="sub-stream %d of %d bytes" % (j, 65535 + k), stored=over and j < 3,
                              sub=(j, 65535 + k), partial=True))
    h = sum(np.bincount(ch, minlength=256) for ch in fixed.values())
    segs[name] = segment(h, [0] * 64, _rng(name), fixed)

    # 16 equiprobable symbols, 4 bits each: all four sub-streams at the limit together (n = 4 * 131 070 and 4 * 131 072)
    name = "edge: 16-bit sizes, 4-bit codes"
    fixed = {}
    for at, n in ((0, 4 * 131070), (63, 4 * 131072)):
        fixed[at] = (16 * 9 + (np.arange(n) * 5) % 16).astype(np.uint8)
        cases.append(dict(segment=name, chunk=at, what="4 x %d bytes" % (n // 8), stored=n // 8 > 0xFFFF, sub=(0, n // 8), partial=True))
    h = sum(np.bincount(ch, minlength=256) for ch in fixed.values())
    segs[name] = segment(h, [0] * 64, _rng(name), fixed)
    return segs, cases


@lru_cache(maxsize=None)
def histogram_segments():
    """every histogram as one segment of 64 chunks of random sizes (some empty)"""
    out = {}
    for name, h in histograms().items():
        rng = _rng(name)
        out[name] = segment(h, [-1] * 64, rng)
    return out


def _end_batch(nchunks, residue):
    """nchunks chunks of one geometric segment whose container total is `residue` (mod 64) with the last record coded: the last chunk
    is short codes, and the first length that lands on the residue is taken"""
    rng = _rng("end %d" % residue)
    head = segment(_geo_counts(4, 10), [-1] * (nchunks - 1), rng) if nchunks > 1 else []
    for n in range(64, 64 + 1200):
        last = np.where(np.arange(n) % 5 == 4, 12, 11).astype(np.uint8)          # two of the segment's most frequent symbols
        chunks = head + [last]
        lens = lengths_model(np.bincount(np.concatenate(chunks), minlength=256))[0]
        total = 0
        for ch in chunks:
            stored, sz = record_sizes(ch, lens)
            total = ((total + 3) & ~3) + (4 + len(ch) if stored else 12 + sum(sz))
        total = (total + 3) & ~3
        if total % 64 == residue and not record_sizes(last, lens)[0]:
            return chunks
    raise AssertionError("no last chunk gives this residue")


@lru_cache(maxsize=None)
def batches():
    """name -> dict(chunks, align, shift, segments = [(segment name, first chunk)], cases = [record cases with their batch chunk index]).
    Chunk counts 1, 63, 64, 65 and 129 among them; containers 16-byte aligned and byte-dense from an odd address."""
    hs, (es, ecases) = histogram_segments(), edge_segments()
    B = {}

    def add(name, seg_names, align, shift, extra=()):
        chunks, segments, cases = [], [], []
        for sn in seg_names:
            segments.append((sn, len(chunks)))
            cases += [dict(c, chunk=c["chunk"] + len(chunks)) for c in ecases if c["segment"] == sn]
            chunks += hs[sn] if sn in hs else es[sn]
        if extra:
            segments.append(("short tail", len(chunks)))
            chunks += list(extra)
        B[name] = dict(chunks=chunks, align=align, shift=shift, segments=segments, cases=cases)

    names = list(hs)
    rng = _rng("tails")
    tail = segment(_geo_counts(1, 200), [-1], rng)                             # (every batch ends in a chunk that is not empty)
    add("histograms, aligned", names[:len(names) // 2], 16, 0, tail)
    add("histograms, byte-dense", names[len(names) // 2:], 1, 1, tail)
    add("edges, 129 chunks, byte-dense", ["edge: stored rule, sizes", "edge: 16-bit sizes, one sub-stream"], 1, 1, tail)
    add("edges, 65 chunks, aligned", ["edge: 16-bit sizes, 4-bit codes"], 16, 0, tail)
    for nchunks, residue in ((63, 0), (64, 4), (1, 60)):
        B["end %d, %d chunks" % (residue, nchunks)] = dict(chunks=_end_batch(nchunks, residue), align=(1, 16, 4)[residue % 3], shift=0,
                                                           segments=[("end %d" % residue, 0)], cases=[], residue=residue)
    return B


def layout(chunks, align, shift=0):
    """-> (dense uint8 with 16 bytes of slack, offsets uint64[n + 1], sizes uint32[n]): chunk starts rounded up to `align`, then moved by
    `shift` bytes; offsets[n] is the end, rounded like a start"""
    n = len(chunks)
    offs = np.zeros(n + 1, np.uint64)
    pos = 0
    for c, ch in enumerate(chunks):
        pos = (pos + align - 1) & ~(align - 1)
        offs[c] = pos + shift
        pos += len(ch)
    offs[n] = ((pos + align - 1) & ~(align - 1)) + shift
    dense = np.full(int(offs[n]) + 16, 0xA5, np.uint8)
    for c, ch in enumerate(chunks):
        dense[int(offs[c]):int(offs[c]) + len(ch)] = ch
    return dense, offs, np.array([len(ch) for ch in chunks], np.uint32)


def segment_counts(chunks, first):
    """the histogram of the segment that starts at chunk `first`"""
    part = [ch for ch in chunks[first:first + SEG] if len(ch)]
    return np.bincount(np.concatenate(part), minlength=256) if part else np.zeros(256, np.int64)


def __getattr__(name):
    if name == "HISTOGRAMS":
        return histograms()
    if name == "RECORD_CASES":
        return [c for b in batches().values() for c in b["cases"]]
    if name == "BATCHES":
        return batches()
    raise AttributeError(name)
