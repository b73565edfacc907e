"""CPU tier of the Huffman drive: tests/huf_drive.py steers the shared code-table builder and the container's writer and reader to
their edges.  Here, without a device: the path-counting model of the code lengths IS the oracle's huf_oracle_lengths on every histogram
tried, the drive REACHES every path it is there for (asserted from the model's statistics, so a histogram that stops getting there
fails here and not silently), three mutants of the specification's tie rules are told apart by it, every record case sits on the side
of its container edge that it claims (read from the oracle's record headers), and an independent bit reader turns the oracle's records
back into the chunks.  The GPU tier (tests/test_gpu_huf_drive.py) runs the kernels on the same batches.  Run with -s for the numbers."""
from functools import lru_cache

import numpy as np
import pytest

import huf_drive as hd
from harness import gen_fuzz, gen_walk
from codec_helpers import check_case, decode_sample


def nibbles(lens):
    lens = np.asarray(lens, np.uint8)
    return (lens[0::2] | (lens[1::2] << 4)).astype(np.uint8)


def line(name, h, st):
    return (f"{name:28s} total {int(np.sum(h)):8d}  nz {st['nz']:3d}  depth {st['depth']:3d}  clamped {st['clamped']:3d}  kraft {st['kraft']:5d}  "
            f"up {st['up']:3d} in quarters {sorted(set(st['up_quarters']))}  down {st['down']:3d} in quarters {sorted(set(st['down_quarters']))}  "
            f"symbol ties up {st['up_symbol_ties']} down {st['down_symbol_ties']}  merge ties 1st {st['merge_ties'][0]} 2nd {st['merge_ties'][1]}")


@lru_cache(maxsize=None)
def stats_of_drive():
    return {name: hd.lengths_model(h) for name, h in hd.histograms().items()}


def random_histograms():
    """the 200 of tests/test_huf_cpu.py::test_lengths_are_a_valid_limited_prefix_code"""
    rng = np.random.default_rng(0)
    for trial in range(200):
        kind = trial % 5
        if kind == 0:
            counts = rng.integers(0, 1000, 256)
        elif kind == 1:
            counts = (rng.random(256) ** 8 * 1e6).astype(np.int64)
        elif kind == 2:
            counts = np.zeros(256, np.int64)
            counts[rng.integers(0, 256, rng.integers(1, 5))] = rng.integers(1, 100)
        elif kind == 3:
            counts = np.ones(256, np.int64)
        else:
            counts = np.array([int(1.6 ** min(i, 40)) for i in range(256)])
        yield "random %d" % trial, counts


def check_table(name, counts, lens):
    """what every table must be, whoever made it: absent <=> 0, at most 11 bits, a complete code from two symbols on"""
    counts, lens = np.asarray(counts), np.asarray(lens).astype(np.int64)
    assert ((lens == 0) == (counts == 0)).all(), name
    assert lens.max() <= hd.LMAX, name
    nz = int((counts > 0).sum())
    kraft = int((1 << (hd.LMAX - lens[lens > 0])).sum())
    if nz >= 2:
        assert kraft == 1 << hd.LMAX, (name, kraft)
    elif nz == 1:
        assert lens.max() == 1, name


def test_the_model_is_the_oracle(oracle):
    for name, h in list(hd.histograms().items()) + list(random_histograms()):
        lens, st = hd.lengths_model(h)
        want = oracle.huf_lengths(h)
        assert np.array_equal(lens, want), (name, "first symbol that differs", int(np.flatnonzero(lens != want)[0]))
        check_table(name, h, lens)
        assert st["nz"] == int((np.asarray(h) > 0).sum())


def test_the_drive_reaches_every_path():
    """Every item of the drive's list, from the model's statistics.  Quarters are the kernel's slot e = (index among the sorted non-zero
    leaves) // 64.  Lengthening moves the deepest codes below 11 bits -- the leaves just behind the clamped ones -- and shortening the most
    frequent ones, so with nz leaves both work in quarter (nz - 1) // 64 or just below: the ladder's nz puts them in all four quarters,
    and all four are asserted for BOTH loops (a search reaches every quarter for shortening too: nz <= 64, <= 128, <= 192, above)."""
    S = {name: st for name, (lens, st) in stats_of_drive().items()}
    H = hd.histograms()
    for name, st in S.items():
        print(line(name, H[name], st))
        assert int(H[name].sum()) <= 4 << 20
    assert [S[k]["nz"] for k in ("no symbol", "one symbol", "two symbols", "three equal")] == [0, 1, 2, 3]
    assert len(set(H["three equal"][H["three equal"] > 0].tolist())) == 1
    d11, d12 = S["depth 11"], S["depth 12"]
    assert (d11["depth"], d11["clamped"], d11["up"], d11["down"], d11["kraft"]) == (11, 0, 0, 0, 2048)
    assert (d12["depth"], d12["up"]) == (12, 1) and d12["clamped"] > 0
    for k in ("fib 24 low", "fib 24 high"):
        assert S[k]["nz"] == 24 and S[k]["depth"] >= 23 and (S[k]["clamped"], S[k]["up"], S[k]["down"]) == (13, 7, 3), S[k]
    assert (H["fib 24 high"][:232] == 0).all() and (H["fib 24 high"][232:] > 0).all()
    ladder = {k: st for k, st in S.items() if k.startswith("ladder")}
    assert sorted(st["nz"] for st in ladder.values()) == [63, 64, 65, 128, 129, 192, 193, 255, 256]
    assert {k.split()[-1] for k in ladder} == {"low", "high", "spread"}
    for k, st in ladder.items():
        assert st["depth"] > hd.LMAX and st["up"] > 0 and st["kraft"] > 2048, (k, st)
    assert max(st["up"] for st in S.values()) >= 40 and S["fib 30 + 226 ones"]["up"] >= 40 and S["powers + 244 ones"]["up"] >= 26
    assert S["shorten search"]["down"] >= 8
    assert S["ties up"]["up_symbol_ties"] > 0 and S["ties up, levels"]["up_symbol_ties"] > 0 and S["ties down"]["down_symbol_ties"] > 0
    assert any(st["merge_ties"][0] for st in S.values()) and any(st["merge_ties"][1] for st in S.values())
    assert {q for st in S.values() for q in st["up_quarters"]} == {0, 1, 2, 3}
    assert {q for st in S.values() for q in st["down_quarters"]} == {0, 1, 2, 3}
    for k in ("all equal", "all ones"):
        assert S[k]["nz"] == 256 and S[k]["depth"] == 8 and S[k]["up"] == S[k]["down"] == 0
    assert (H["all ones"] == 1).all()


@pytest.mark.parametrize("mutant", list(hd.MUTANTS))
def test_the_drive_tells_the_mutants_apart(oracle, mutant):
    """a builder with one tie rule of the specification turned round differs from the oracle's table on a drive histogram"""
    caught = [name for name, h in hd.histograms().items()
              if not np.array_equal(hd.lengths_model(h, **hd.MUTANTS[mutant])[0], oracle.huf_lengths(h))]
    print(f"mutant '{mutant}' caught by: {caught}")
    assert caught


def test_the_segments_hold_their_histograms():
    """what K1 will count in every segment of every batch IS the named histogram; the drive stays in its budget; the chunk counts and
    source alignments of the list are there"""
    H, B = hd.histograms(), hd.batches()
    seen, total = set(), 0
    for bname, b in B.items():
        total += sum(len(ch) for ch in b["chunks"])
        for sname, first in b["segments"]:
            if sname in H:
                assert np.array_equal(hd.segment_counts(b["chunks"], first), H[sname]), (bname, sname)
                seen.add(sname)
    assert seen == set(H)
    assert total <= 16 << 20
    assert {1, 63, 64, 65, 129} <= {len(b["chunks"]) for b in B.values()}
    assert {b["align"] for b in B.values()} >= {1, 16} and any(b["shift"] & 1 for b in B.values())
    print(f"drive: {len(B)} batches, {sum((len(b['chunks']) + 63) // 64 for b in B.values())} segments, {total} bytes")


@lru_cache(maxsize=None)
def oracle_container(oracle, bname):
    b = hd.batches()[bname]
    dense, offs, sizes = hd.layout(b["chunks"], b["align"], b["shift"])
    huf, ho, tables = oracle.huf_compress(dense, offs, sizes)
    return huf, ho, tables


@pytest.mark.parametrize("bname", list(hd.batches()))
def test_oracle_records_sit_on_their_edges_and_decode(oracle, bname):
    b = hd.batches()[bname]
    huf, ho, tables = oracle_container(oracle, bname)
    assert ho[-1] == huf.size and (ho % 4 == 0).all()
    for sname, first in b["segments"]:                                           # the tables are the model's
        lens = hd.lengths_model(hd.segment_counts(b["chunks"], first))[0]
        assert np.array_equal(tables[128 * (first // 64):128 * (first // 64) + 128], nibbles(lens)), (bname, sname)
    for case in b["cases"]:
        check_case(case, b["chunks"][case["chunk"]], huf, ho, tables)
        print(f"{bname}: chunk {case['chunk']:3d} '{case['what']}' -> header {hd.record_header(huf[int(ho[case['chunk']]):])}")
    if "residue" in b:
        assert huf.size % 64 == b["residue"] and not hd.record_header(huf[int(ho[-2]):])[1], (bname, huf.size)
        # what the reader's 16-byte piece loads may touch lies inside what huf_bound promises (total + 8 * nchunks + 16)
        total_in = sum(len(ch) for ch in b["chunks"])
        assert ((huf.size + 15) & ~15) <= total_in + 8 * len(b["chunks"]) + 16
    done = decode_sample(b, huf, ho, tables)
    print(f"{bname}: {done} symbols through decode_record")


@pytest.mark.parametrize("bname", ["histograms, aligned", "edges, 129 chunks, byte-dense", "end 60, 1 chunks"])
def test_oracle_reader_at_every_alignment(oracle, bname):
    """the specification of the reader's `align`: chunk starts and the end rounded up, every chunk back"""
    b = hd.batches()[bname]
    huf, ho, tables = oracle_container(oracle, bname)
    for align in (1, 2, 4, 8, 16):
        want_offs = hd.layout(b["chunks"], align)[1]
        back, offs, sizes = oracle.huf_decompress(huf, ho, tables, int(want_offs[-1]), align=align)
        assert np.array_equal(offs, want_offs) and back.size == int(want_offs[-1]), (bname, align)
        assert np.array_equal(sizes, [len(ch) for ch in b["chunks"]])
        for c, ch in enumerate(b["chunks"]):
            assert np.array_equal(back[int(offs[c]):int(offs[c]) + len(ch)], ch), (bname, align, c)


def test_every_record_case_of_the_list_is_there():
    whats = [c["what"] for b in hd.batches().values() for c in b["cases"]]
    for w in ["enc == n - 9", "enc == n - 8", "4 x 65535 bytes", "4 x 65536 bytes"] + ["size %d" % s for s in hd.SMALL_SIZES] + \
            ["sub-stream %d of %d bytes" % (j, s) for j in range(4) for s in (65535, 65536)]:
        assert w in whats, w
    assert sorted(b["residue"] for b in hd.batches().values() if "residue" in b) == [0, 4, 60]


# ----------------------------------------------------------------- what the natural inputs of the existing GPU tests reach

def natural_histograms(oracle):
    """the segments that tests/test_gpu_parity.py::test_huffman_stage_matches_oracle_and_roundtrips and
    tests/test_gpu_huf0.py::test_writer_edge_chunks feed K1, with those tests' own seeds (the GPU encoder's streams are the oracle's)"""
    for step in (2, 8, 300):
        rng = np.random.default_rng(40 + step)
        data = np.concatenate([gen_walk(rng, 100 * 5120, 8, 2, step, flat_every=5), gen_fuzz(rng, 50 * 5120, 2, 0)])
        streams = oracle.compress_chunks("xff", data, 5120, 8)
        for first in range(0, len(streams), 64):
            yield "stage step %d segment %d" % (step, first // 64), hd.segment_counts(streams, first)
    rng = np.random.default_rng(77)
    chunks = []
    for n in (0, 1, 2, 11, 12, 13, 40, 300, 4096, 70000, 300000):
        for k in (1, 2, 5, 60, 256):
            p = 1.0 / np.arange(1, k + 1) ** 1.5
            chunks.append(rng.choice(k, n, p=p / p.sum()).astype(np.uint8))
    chunks.append(rng.integers(0, 256, 5000).astype(np.uint8))
    chunks.append(np.full(9000, 7, np.uint8))
    order = rng.permutation(len(chunks))
    chunks = [chunks[i] for i in order] * 3
    for first in range(0, len(chunks), 64):
        yield "edge chunks segment %d" % (first // 64), hd.segment_counts(chunks, first)


def test_paths_the_natural_inputs_reach(oracle):
    """On record: before the drive, K1 saw on the GPU no segment of fewer than 100 symbols, no depth of 23, never 8 shortening rounds
    (two, on one histogram three times), no shortening round decided by the symbol alone, no lengthening in the 64-leaf quarters 0 and
    2 and no shortening outside quarter 3."""
    S = {}
    for name, h in natural_histograms(oracle):
        lens, st = hd.lengths_model(h)
        assert np.array_equal(lens, oracle.huf_lengths(h)), name
        S[name] = st
        print(line(name, h, st))
    assert len(S) == 12
    assert min(st["nz"] for st in S.values()) >= 100                          # not reached: 0, 1, 2, few symbols
    assert max(st["depth"] for st in S.values()) < 23                         # not reached: a depth well beyond 16
    assert max(st["down"] for st in S.values()) < 8                           # not reached: a long shortening loop
    assert sum(st["down_symbol_ties"] for st in S.values()) == 0              # not reached: a shortening tie decided by the symbol
    assert not {q for st in S.values() for q in st["up_quarters"]} & {0, 2}   # not reached: lengthening in slots e = 0, 2
    assert {q for st in S.values() for q in st["down_quarters"]} <= {3}       # not reached: shortening in slots e = 0, 1, 2
    assert max(st["up"] for st in S.values()) > 0                             # reached: the lengthening loop
