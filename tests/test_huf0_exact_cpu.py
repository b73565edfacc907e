"""The exact Huff0 writer's specification, CPU side: tests/huf0_exact_model.py (a restatement of libzstd
1.4.8's HUF_compress2) against the committed libzstd blocks and against the live library."""
import numpy as np
import pytest

from harness import Zstd
from huf0_exact_model import fse_normalize, fse_optimal_table_log, huf_compress_exact


def _zstd():
    try:
        z = Zstd()
        z.z.HUF_compress2
    except (OSError, AttributeError):
        pytest.skip("no libzstd with HUF_compress on this machine")
    return z


def test_model_reproduces_the_committed_blocks(golden_huf0):
    manifest, arrays = golden_huf0
    assert len(manifest) == 372
    stats = {}
    for m in manifest:
        plain, blk = arrays["p%04d" % m["idx"]], arrays["b%04d" % m["idx"]]
        got = huf_compress_exact(plain, 12 if m["name"].startswith("log12") else 11, stats)
        assert got.size == blk.size and np.array_equal(got, blk), m
    assert stats["fse"] == 208 and stats["nibbles"] == 36 and stats["set_max_height"] > 100


def _zipf(rng, n, k, s):
    p = 1.0 / np.arange(1, k + 1) ** s
    sym = rng.permutation(256)[:k]
    return sym[rng.choice(k, n, p=p / p.sum())].astype(np.uint8)


def _from_counts(rng, counts, shuffle=True):
    x = np.repeat(np.arange(len(counts)), counts).astype(np.uint8)
    return rng.permutation(x) if shuffle else x


def _m2_weight_profiles(rng, want):
    """weight histograms (table log 12, Kraft-complete once the implied last symbol is added) for which
    FSE_normalizeCount falls back to FSE_normalizeM2: a search in weight space (~1 in 15 000 draws)"""
    out = []
    while len(out) < want:
        budget, c = 1 << 12, np.zeros(13, np.int64)
        for w in range(12, 1, -1):
            c[w] = rng.integers(0, min(budget >> (w - 1), int(rng.integers(1, 40))) + 1)
            budget -= int(c[w]) << (w - 1)
        c[1], c[0] = budget - 1, rng.integers(0, 60)        # one weight-1 symbol is the last one: its weight is implied
        nw = int(c.sum())
        if c[1] < 0 or c[12] == 0 or not 3 <= nw <= 254 or c.max() in (1, nw):
            continue
        maxw, st = int(np.nonzero(c)[0].max()), {}
        fse_normalize(c, fse_optimal_table_log(6, nw, maxw, 2), nw, maxw, st)
        if st.get("normalize_m2"):
            out.append(c)
    return out


def generated_inputs(rng):
    """(family, bytes) pairs; the families the acceptance list names"""
    for _ in range(2000):                                  # random Zipf skews
        n = int(rng.choice([16, 40, 100, 300, 1000, 2600, 5000, 20000]))
        yield "zipf", _zipf(rng, n, int(rng.integers(2, 257)), float(rng.uniform(0.3, 3.0)))
    for _ in range(400):                                   # Fibonacci-like counts: lengths past 11, setMaxHeight
        k = int(rng.integers(14, 30))
        f = [1, 1]
        while len(f) < k:
            f.append(f[-1] + f[-2])
        c = np.array(f[:k], np.int64)
        while c.sum() > 120000:
            c = np.maximum(c // 2, 1)
        c = c + rng.integers(0, 3, size=k)
        counts = np.zeros(256, np.int64)
        counts[rng.permutation(256)[:k]] = c
        yield "fib", _from_counts(rng, counts)
    for _ in range(800):                                   # near-equal counts: tie order
        k = int(rng.integers(2, 257))
        base = int(rng.integers(3, 60))
        counts = np.zeros(256, np.int64)
        counts[rng.permutation(256)[:k]] = base + rng.integers(0, 3, size=k)
        if rng.random() < 0.5:
            counts[int(rng.integers(0, 256))] += base * int(rng.integers(2, 40))
        yield "ties", _from_counts(rng, counts)
    for _ in range(1600):                                  # weight distributions searched for the low-probability and normalizeM2 paths
        k = int(rng.integers(40, 257))
        counts = np.zeros(256, np.int64)
        heavy = int(rng.integers(1, 8))
        counts[:k] = rng.integers(1, 4, size=k)
        counts[rng.permutation(k)[:heavy]] = rng.integers(200, 6000, size=heavy)
        yield "weights", _from_counts(rng, counts)
    for c in _m2_weight_profiles(rng, 12):                 # ... and inputs whose code has those weights (dyadic counts x 3)
        ws = rng.permutation(np.repeat(np.arange(13), c))
        counts = np.array([0 if w == 0 else 3 << (w - 1) for w in ws] + [3], np.int64)
        yield "m2_log12", _from_counts(rng, counts)
    for _ in range(300):                                   # small alphabets: the 4-bit description
        k = int(rng.integers(3, 40))
        p = 1.0 / np.arange(1, k + 1) ** float(rng.uniform(0.5, 2.0))
        yield "small", rng.choice(k, int(rng.choice([100, 1000, 6000])), p=p / p.sum()).astype(np.uint8)
    for k in (2, 128, 129, 256):                           # distinct-symbol counts
        for _ in range(60):
            n = int(rng.choice([300, 3000, 30000]))
            sym = rng.permutation(256)[:k]
            p = 1.0 / np.arange(1, k + 1) ** float(rng.uniform(0.0, 2.0))
            x = sym[rng.choice(k, n, p=p / p.sum())].astype(np.uint8)
            x[:k] = sym                                    # every one of the k symbols present
            yield f"k{k}", x
    for n in (0, 1, 11, 12, 13, 128 * 1024, 128 * 1024 + 1):   # sizes
        for s in (0.5, 1.2, 2.5):
            yield f"n{n}", _zipf(rng, n, 50, s)


def test_model_equals_libzstd_on_generated_inputs():
    z = _zstd()
    if z.version != 10408:
        pytest.skip(f"the model is of libzstd 1.4.8; this machine has {z.version}")
    rng = np.random.default_rng(20240)
    stats, fam, n_cases = {}, {}, 0
    for family, data in generated_inputs(rng):
        for tl in ((11, 12) if family.startswith("n") else (12,) if family.endswith("log12") else (11,)):
            want = z.huf_compress(data, tl)
            got = huf_compress_exact(data, tl, stats)
            assert got.size == want.size and np.array_equal(got, want), (family, data.size, tl)
            n_cases += 1
        fam[family] = fam.get(family, 0) + 1
    print(f"{n_cases} inputs; families {fam}; paths {stats}")
    assert n_cases >= 5000
    assert stats.get("set_max_height", 0) > 100 and stats.get("low_prob", 0) > 100 and stats.get("normalize_m2", 0) > 0
    assert stats["normalize_m2"] >= 12 and stats.get("fse", 0) > 1000 and stats.get("nibbles", 0) > 50
