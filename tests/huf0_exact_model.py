"""A numpy/Python model of libzstd 1.4.8's HUF_compress2(dst, bound, src, n, 255, table_log): the
specification of the exact Huff0 writer (sprintz_mi355x_huf0_compress_batch_exact, csrc/huf0_exact.h).
Test infrastructure.  The authority is the library itself (tests/test_huf0_exact_cpu.py checks the model
against it and against tests/golden/golden_huf0_v1); the stages follow huf_compress.c / fse_compress.c.

huf_compress_exact(data, table_log) returns the block with tests/harness.py:Zstd.huf_compress's
conventions: the input itself when HUF_compress declines, one byte for a single repeated symbol,
nothing for an empty input.  `stats` (a dict, optional) counts the rarer paths the model took."""
import numpy as np

BLOCKSIZE_MAX = 128 * 1024
TABLELOG_MAX = 12


def highbit(v):
    return int(v).bit_length() - 1


def fse_optimal_table_log(max_log, n, max_sym, minus):
    """FSE_optimalTableLog_internal"""
    max_bits_src = (highbit(n - 1) - minus) & 0xFFFFFFFF      # (unsigned: wraps for tiny n)
    log = max_log
    min_bits = min(highbit(n) + 1, highbit(max_sym) + 2)      # FSE_minTableLog
    if max_bits_src < log:
        log = max_bits_src
    if min_bits > log:
        log = min_bits
    return min(max(log, 5), 12)


def huf_optimal_table_log(max_log, n, max_sym):
    return fse_optimal_table_log(max_log, n, max_sym, 1)


# ------------------------------------------------------------------ code lengths (HUF_buildCTable)

def huf_sort(count, max_sym):
    """symbols by count descending, equal counts in ascending symbol order (HUF_sort's result)"""
    syms = list(range(max_sym + 1))
    syms.sort(key=lambda s: (-int(count[s]), s))
    return syms


def huf_set_max_height(nb, cnt, last_non_null, max_nb_bits):
    """HUF_setMaxHeight on the sorted node arrays nb (lengths) / cnt (counts); nb is changed in place"""
    largest = nb[last_non_null]
    if largest <= max_nb_bits:
        return largest
    total_cost = 0
    base_cost = 1 << (largest - max_nb_bits)
    n = last_non_null
    while nb[n] > max_nb_bits:
        total_cost += base_cost - (1 << (largest - nb[n]))
        nb[n] = max_nb_bits
        n -= 1
    while nb[n] == max_nb_bits:
        n -= 1
    total_cost >>= largest - max_nb_bits
    NO = None
    rank_last = [NO] * (TABLELOG_MAX + 2)
    cur = max_nb_bits
    for pos in range(n, -1, -1):
        if nb[pos] >= cur:
            continue
        cur = nb[pos]
        rank_last[max_nb_bits - cur] = pos
    while total_cost > 0:
        dec = highbit(total_cost) + 1
        while dec > 1:
            hi, lo = rank_last[dec], rank_last[dec - 1]
            if hi is NO:
                dec -= 1
                continue
            if lo is NO:
                break
            if cnt[hi] <= 2 * cnt[lo]:
                break
            dec -= 1
        while dec <= TABLELOG_MAX and rank_last[dec] is NO:
            dec += 1
        total_cost -= 1 << (dec - 1)
        if rank_last[dec - 1] is NO:
            rank_last[dec - 1] = rank_last[dec]
        nb[rank_last[dec]] += 1
        if rank_last[dec] == 0:
            rank_last[dec] = NO
        else:
            rank_last[dec] -= 1
            if nb[rank_last[dec]] != max_nb_bits - dec:
                rank_last[dec] = NO
    while total_cost < 0:
        if rank_last[1] is NO:
            while nb[n] == max_nb_bits:
                n -= 1
            nb[n + 1] -= 1
            rank_last[1] = n + 1
            total_cost += 1
            continue
        nb[rank_last[1] + 1] -= 1
        rank_last[1] += 1
        total_cost += 1
    return max_nb_bits


def huf_build_lengths(count, max_sym, max_nb_bits, stats=None):
    """-> (lengths per symbol 0..255, the table log = the longest length)"""
    order = huf_sort(count, max_sym)
    cnt = [int(count[s]) for s in order]
    last = max_sym
    while cnt[last] == 0:
        last -= 1
    # two-queue merge: leaves last .. 0 (ascending counts), internal nodes in creation order
    nleaf = last + 1
    ncnt = [0] * nleaf                 # internal node counts
    parent_leaf = [0] * nleaf
    parent_node = [0] * nleaf
    ncnt[0] = cnt[last] + cnt[last - 1]
    parent_leaf[last] = parent_leaf[last - 1] = 0
    nn, low_s, low_n = 1, last - 2, 0
    big = 1 << 30
    while nn < nleaf - 1:
        picks = []
        for _ in range(2):
            cs = cnt[low_s] if low_s >= 0 else 1 << 31
            cn = ncnt[low_n] if low_n < nn else big
            if cs < cn:
                picks.append(("s", low_s))
                low_s -= 1
            else:
                picks.append(("n", low_n))
                low_n += 1
        ncnt[nn] = sum(cnt[i] if k == "s" else ncnt[i] for k, i in picks)
        for k, i in picks:
            (parent_leaf if k == "s" else parent_node)[i] = nn
        nn += 1
    root = nleaf - 2
    depth = [0] * (nleaf - 1)
    for i in range(root - 1, -1, -1):
        depth[i] = depth[parent_node[i]] + 1
    nb = [depth[parent_leaf[i]] + 1 for i in range(nleaf)]
    if stats is not None and nb[last] > max_nb_bits:
        stats["set_max_height"] = stats.get("set_max_height", 0) + 1
    tl = huf_set_max_height(nb, cnt, last, max_nb_bits)
    lens = np.zeros(256, np.int64)
    for i in range(nleaf):
        lens[order[i]] = nb[i]
    return lens, tl


def huf_code_values(lens, tl):
    """canonical code values (HUF_buildCTable): per length, ascending symbols; the longest codes lowest"""
    per = np.bincount(lens, minlength=16)
    start = [0] * 16
    m = 0
    for l in range(tl, 0, -1):
        start[l] = m
        m = (m + int(per[l])) >> 1
    vals = np.zeros(256, np.int64)
    for s in range(256):
        l = int(lens[s])
        if l:
            vals[s] = start[l]
            start[l] += 1
    return vals


# ------------------------------------------------------------------ tree description (HUF_writeCTable)

def fse_normalize(count, table_log, total, max_sym, stats=None):
    """FSE_normalizeCount with useLowProbCount = 0 (HUF_compressWeights' call): low-probability symbols get 1"""
    low_prob = 1
    rtb = [0, 473195, 504333, 520860, 550000, 700000, 750000, 830000]
    scale = 62 - table_log
    step = (1 << 62) // total
    vstep = 1 << (scale - 20)
    still = 1 << table_log
    largest, largest_p = 0, 0
    low_threshold = total >> table_log
    norm = [0] * (max_sym + 1)
    for s in range(max_sym + 1):
        c = int(count[s])
        if c == total:
            return None                     # (rle: never reached from HUF_compressWeights)
        if c == 0:
            continue
        if c <= low_threshold:
            norm[s] = low_prob
            still -= 1
            if stats is not None:
                stats["low_prob"] = stats.get("low_prob", 0) + 1
        else:
            proba = (c * step) >> scale
            if proba < 8:
                rest = vstep * rtb[proba]
                proba += (c * step) - (proba << scale) > rest
            if proba > largest_p:
                largest_p, largest = proba, s
            norm[s] = proba
            still -= proba
    if -still >= (norm[largest] >> 1):
        if stats is not None:
            stats["normalize_m2"] = stats.get("normalize_m2", 0) + 1
        return fse_normalize_m2(count, table_log, total, max_sym, low_prob)
    norm[largest] += still
    return norm


def fse_normalize_m2(count, table_log, total, max_sym, low_prob):
    NA = -2
    norm = [0] * (max_sym + 1)
    distributed = 0
    low_threshold = total >> table_log
    low_one = (total * 3) >> (table_log + 1)
    for s in range(max_sym + 1):
        c = int(count[s])
        if c == 0:
            continue
        if c <= low_threshold:
            norm[s] = low_prob
            distributed += 1
            total -= c
            continue
        if c <= low_one:
            norm[s] = 1
            distributed += 1
            total -= c
            continue
        norm[s] = NA
    to_dist = (1 << table_log) - distributed
    if to_dist == 0:
        return norm
    if total // to_dist > low_one:
        low_one = (total * 3) // (to_dist * 2)
        for s in range(max_sym + 1):
            if norm[s] == NA and int(count[s]) <= low_one:
                norm[s] = 1
                distributed += 1
                total -= int(count[s])
        to_dist = (1 << table_log) - distributed
    if distributed == max_sym + 1:
        max_v, max_c = 0, 0
        for s in range(max_sym + 1):
            if int(count[s]) > max_c:
                max_v, max_c = s, int(count[s])
        norm[max_v] += to_dist
        return norm
    if total == 0:
        s = 0
        while to_dist > 0:
            if norm[s] > 0:
                to_dist -= 1
                norm[s] += 1
            s = (s + 1) % (max_sym + 1)
        return norm
    vlog = 62 - table_log
    mid = (1 << (vlog - 1)) - 1
    rstep = (((1 << vlog) * to_dist) + mid) // total
    tmp = mid
    for s in range(max_sym + 1):
        if norm[s] == NA:
            end = tmp + int(count[s]) * rstep
            w = (end >> vlog) - (tmp >> vlog)
            if w < 1:
                return None
            norm[s] = w
            tmp = end
    return norm


class BitW:
    def __init__(self):
        self.bits = []                      # (value, nbits), LSB first

    def add(self, v, nb):
        self.bits.append((int(v) & ((1 << nb) - 1), nb))

    def nbits(self):
        return sum(nb for _, nb in self.bits)

    def tobytes(self):
        acc, n = 0, 0
        for v, nb in self.bits:
            acc |= v << n
            n += nb
        return np.frombuffer(acc.to_bytes((n + 7) // 8, "little"), np.uint8).copy() if n else np.zeros(0, np.uint8)


def fse_write_ncount(norm, max_sym, table_log):
    """FSE_writeNCount -> bytes, or None (incorrect distribution)"""
    bw = BitW()
    bw.add(table_log - 5, 4)
    remaining = (1 << table_log) + 1
    threshold = 1 << table_log
    nbits = table_log + 1
    sym, prev0 = 0, False
    alpha = max_sym + 1
    while sym < alpha and remaining > 1:
        if prev0:
            start = sym
            while sym < alpha and not norm[sym]:
                sym += 1
            if sym == alpha:
                break
            while sym >= start + 24:
                start += 24
                bw.add(0xFFFF, 16)
            while sym >= start + 3:
                start += 3
                bw.add(3, 2)
            bw.add(sym - start, 2)
        c = norm[sym]
        sym += 1
        mx = (2 * threshold - 1) - remaining
        remaining -= abs(c)
        c += 1
        if c >= threshold:
            c += mx
        bw.add(c, nbits - (c < mx))
        prev0 = c == 1
        if remaining < 1:
            return None
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
    if remaining != 1:
        return None
    return bw.tobytes()


def fse_compress(src, norm, max_sym, table_log):
    """FSE_buildCTable + FSE_compress_usingCTable (two interleaved states, last symbol first) -> bytes, or None"""
    n = len(src)
    if n <= 2:
        return None
    size = 1 << table_log
    mask = size - 1
    step = (size >> 1) + (size >> 3) + 3
    high = size - 1
    table_sym = [0] * size
    cumul = [0] * (max_sym + 2)
    for u in range(1, max_sym + 2):
        if norm[u - 1] == -1:
            cumul[u] = cumul[u - 1] + 1
            table_sym[high] = u - 1
            high -= 1
        else:
            cumul[u] = cumul[u - 1] + norm[u - 1]
    pos = 0
    for s in range(max_sym + 1):
        for _ in range(max(norm[s], 0)):
            table_sym[pos] = s
            pos = (pos + step) & mask
            while pos > high:
                pos = (pos + step) & mask
    assert pos == 0
    state_table = [0] * size
    cum = list(cumul)
    for u in range(size):
        s = table_sym[u]
        state_table[cum[s]] = size + u
        cum[s] += 1
    dnb, dfs = [0] * (max_sym + 1), [0] * (max_sym + 1)
    total = 0
    for s in range(max_sym + 1):
        c = norm[s]
        if c == 0:
            dnb[s] = ((table_log + 1) << 16) - size
        elif c in (-1, 1):
            dnb[s] = (table_log << 16) - size
            dfs[s] = total - 1
            total += 1
        else:
            mbo = table_log - highbit(c - 1)
            dnb[s] = (mbo << 16) - (c << mbo)
            dfs[s] = total - c
            total += c
    bw = BitW()

    def init(sym):
        nbo = (dnb[sym] + (1 << 15)) >> 16
        v = (nbo << 16) - dnb[sym]
        return state_table[(v >> nbo) + dfs[sym]]

    def enc(st, sym):
        nbo = (st + dnb[sym]) >> 16
        bw.add(st, nbo)
        return state_table[(st >> nbo) + dfs[sym]]

    i = n
    if n & 1:
        s1 = init(src[i - 1]); s2 = init(src[i - 2]); i -= 2
        s1 = enc(s1, src[i - 1]); i -= 1
    else:
        s2 = init(src[i - 1]); s1 = init(src[i - 2]); i -= 2
    while i > 0:                       # (pairs; the 64-bit container's grouping does not change the bit order)
        s2 = enc(s2, src[i - 1])
        s1 = enc(s1, src[i - 2])
        i -= 2
    bw.add(s2, table_log)
    bw.add(s1, table_log)
    bw.add(1, 1)
    return bw.tobytes()


def huf_compress_weights(weights, stats=None):
    """HUF_compressWeights -> (hSize, bytes); hSize 0 / 1 = not compressible / rle"""
    wt = len(weights)
    if wt <= 1:
        return 0, None
    count = np.bincount(np.asarray(weights, np.int64), minlength=13)
    max_w = int(np.nonzero(count)[0].max())
    max_count = int(count.max())
    if max_count == wt:
        return 1, None
    if max_count == 1:
        return 0, None
    tl = fse_optimal_table_log(6, wt, max_w, 2)
    norm = fse_normalize(count, tl, wt, max_w, stats)
    if norm is None:
        return -1, None
    hdr = fse_write_ncount(norm, max_w, tl)
    if hdr is None:
        return -1, None
    body = fse_compress(list(weights), norm, max_w, tl)
    if body is None:
        return 0, None
    out = np.concatenate([hdr, body])
    return out.size, out


def huf_write_ctable(lens, max_sym, tl, stats=None):
    """HUF_writeCTable -> description bytes, or None (HUF_compress fails: the chunk is stored)"""
    w = [(tl + 1 - int(lens[s])) if lens[s] else 0 for s in range(max_sym)]
    hsize, body = huf_compress_weights(w, stats)
    if hsize < 0:
        return None
    if 1 < hsize < max_sym // 2:
        return np.concatenate([np.array([hsize], np.uint8), body])
    if max_sym > 128:
        return None
    w.append(0)
    out = [128 + max_sym - 1] + [(w[k] << 4) + w[k + 1] for k in range(0, max_sym, 2)]
    return np.array(out, np.uint8)


# ------------------------------------------------------------------ streams

def encode_stream(seg, vals, lens):
    """one stream: symbols last first, LSB-first bit packing, the closing 1 bit"""
    if seg.size == 0:
        return np.array([1], np.uint8)
    s = seg[::-1].astype(np.int64)
    v, l = vals[s], lens[s]
    total = int(l.sum()) + 1
    nbytes = (total + 7) // 8
    pos = np.concatenate([[0], np.cumsum(l)[:-1]])
    maxl = int(l.max())
    bits = np.zeros(nbytes * 8, np.uint8)
    for b in range(maxl):
        m = l > b
        bits[pos[m] + b] = (v[m] >> b) & 1
    bits[total - 1] = 1
    return np.packbits(bits, bitorder="little")


def huf_compress_exact(data, table_log=11, stats=None):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    if n == 0:
        return data.copy()
    stored = data.copy()
    if n > BLOCKSIZE_MAX:
        return stored
    count = np.bincount(data, minlength=256)
    max_sym = int(np.nonzero(count)[0].max())
    largest = int(count.max())
    if largest == n:
        return data[:1].copy()
    if largest <= (n >> 7) + 4:
        return stored
    tl = huf_optimal_table_log(table_log, n, max_sym)
    lens, tl = huf_build_lengths(count, max_sym, tl, stats)
    if tl > TABLELOG_MAX:
        return stored
    hdr = huf_write_ctable(lens, max_sym, tl, stats)
    if hdr is None:
        return stored
    if hdr.size + 12 >= n:
        return stored
    if n < 12:
        return stored
    vals = huf_code_values(lens, tl)
    q = (n + 3) // 4
    streams = [encode_stream(data[k * q: min((k + 1) * q, n)], vals, lens) for k in range(4)]
    jt = np.array([streams[0].size & 255, streams[0].size >> 8, streams[1].size & 255, streams[1].size >> 8,
                   streams[2].size & 255, streams[2].size >> 8], np.uint8)
    out = np.concatenate([hdr, jt] + streams)
    if out.size >= n - 1:
        return stored
    if stats is not None:
        kind = "fse" if hdr[0] < 128 else "nibbles"
        stats[kind] = stats.get(kind, 0) + 1
    return out
