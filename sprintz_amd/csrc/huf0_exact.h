// huf0_exact.h -- the exact Huff0 writer (included by huf.hip inside its anonymous namespace, after huf0_write.h):
// per chunk, byte for byte what libzstd 1.4.8's HUF_compress2(dst, bound, src, n, 255, table_log) returns, with
// Zstd.huf_compress's conventions (declined -> the chunk verbatim, one repeated byte -> that byte, empty -> empty).
// Specification: tests/huf0_exact_model.py, itself checked against the library.  Every chunk has its own code table.
//   X1 huf0x_table_kernel   one wave per chunk: four per-stream histograms in LDS, the early exits, HUF_optimalTableLog,
//                           the sort (parallel ranks), the two-queue merge + HUF_setMaxHeight + HUF_writeCTable (lane 0),
//                           the canonical code values, the four streams' byte counts from the histograms -> record, size, meta
//   (launch_size_scan)      block sizes -> byte-dense block offsets
//   X2 huf0x_encode_kernel  16 chunks a wave, lane = (chunk, stream): description, jump table, streams last symbol first
#pragma once

// per-chunk record (X1 -> X2): hlen u32 @0 | tableLog u32 @4 | tree description, <= 128 bytes @8 | code 256 x u16 (value | length << 12) @144
constexpr int kXRecBytes = 656, kXRecHdr = 8, kXRecTab = 144;
constexpr uint32_t kXBlockMax = 128u * 1024u;          // HUF_BLOCKSIZE_MAX: larger chunks are stored

__device__ __forceinline__ uint32_t highbit32(uint32_t v) { return 31u - (uint32_t)__clz((int)v); }

// FSE_optimalTableLog_internal (unsigned arithmetic as in the library: maxBitsSrc wraps for tiny inputs)
__device__ __forceinline__ uint32_t fse_optimal_table_log(uint32_t max_log, uint32_t n, uint32_t max_sym, uint32_t minus)
{
    const uint32_t max_bits_src = highbit32(n - 1u) - minus;
    uint32_t log = max_log;
    const uint32_t a = highbit32(n) + 1u, b = highbit32(max_sym ? max_sym : 1u) + 2u - (max_sym ? 0u : 2u);
    const uint32_t min_bits = a < b ? a : b;
    if (max_bits_src < log) log = max_bits_src;
    if (min_bits > log) log = min_bits;
    if (log < 5u) log = 5u;
    if (log > 12u) log = 12u;
    return log;
}

__global__ void __launch_bounds__(64) huf0x_table_kernel(const uint8_t* __restrict__ dense, const uint64_t* __restrict__ offsets,
                                                         const uint32_t* __restrict__ sizes, uint32_t table_log,
                                                         uint8_t* __restrict__ recs, uint32_t* __restrict__ bsizes,
                                                         uint64_t* __restrict__ meta)
{
    __shared__ uint32_t hist[4][256];                  // per stream
    __shared__ uint32_t cnt[256];                      // per symbol
    __shared__ uint32_t scnt[256];                     // sorted: count descending, equal counts ascending symbol
    __shared__ uint8_t ssym[256];
    __shared__ uint32_t ncnt[256];                     // internal nodes' counts, in creation order
    __shared__ uint8_t pleaf[256], pnode[256], depth[256], nb[256], lens[256], wts[256];
    __shared__ uint16_t code[256];
    __shared__ uint8_t hdr[192];
    __shared__ uint32_t rank_last[16];
    __shared__ uint32_t wcnt[16];
    __shared__ int wnorm[16];
    __shared__ uint8_t tsym[64];
    __shared__ uint16_t stab[64];
    __shared__ uint32_t s_tl, s_hlen;
    const int t = threadIdx.x;
    const uint64_t c = blockIdx.x;
    const uint32_t n = sizes[c];
    const uint8_t* const s = dense + offsets[c];
    uint8_t* const rec = recs + c * kXRecBytes;
    for (int k = t; k < 4 * 256; k += 64) (&hist[0][0])[k] = 0;
    __syncthreads();
    // ---- histogram (one per stream: the streams' byte counts follow from it once the lengths are known)
    const uint32_t q = (n + 3u) >> 2;
    if (n <= kXBlockMax)
        for (uint32_t k = (uint32_t)t; k < n; k += 64) atomicAdd(&hist[k / q][s[k]], 1u);
    __syncthreads();
    uint32_t largest_l = 0, ms_l = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int sy = 4 * t + e;
        const uint32_t v = hist[0][sy] + hist[1][sy] + hist[2][sy] + hist[3][sy];
        cnt[sy] = v;
        largest_l = v > largest_l ? v : largest_l;
        if (v) ms_l = (uint32_t)sy + 1u;
    }
    const uint32_t largest = wave_max32(largest_l), max_sym1 = wave_max32(ms_l);
    // mode 0 empty, 1 stored, 2 one repeated byte, 3 coded (huf0_size_kernel's meta)
    uint32_t mode = n == 0 ? 0u : n > kXBlockMax ? 1u : largest == n ? 2u : largest <= (n >> 7) + 4u ? 1u : 3u;
    if (mode == 3) {
        const uint32_t max_sym = max_sym1 - 1u;
        __syncthreads();
        // ---- HUF_sort's order: a symbol's place = symbols with a larger count + symbols with the same count and a smaller index
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t sy = (uint32_t)(4 * t + e);
            if (sy > max_sym) continue;
            const uint32_t v = cnt[sy];
            uint32_t pos = 0;
            for (uint32_t o = 0; o <= max_sym; o++) { const uint32_t w = cnt[o]; pos += (w > v) || (w == v && o < sy); }
            scnt[pos] = v;
            ssym[pos] = (uint8_t)sy;
        }
        __syncthreads();
        if (t == 0) {
            // ---- HUF_buildCTable: the two-queue merge (ties take the internal node), depths, HUF_setMaxHeight
            uint32_t last = max_sym;
            while (scnt[last] == 0) last--;
            const uint32_t nleaf = last + 1u;
            ncnt[0] = scnt[last] + scnt[last - 1];
            pleaf[last] = 0; pleaf[last - 1] = 0;
            int low_s = (int)last - 2;
            uint32_t low_n = 0, nn = 1;
            while (nn < nleaf - 1u) {
                uint32_t sum = 0;
                for (int r = 0; r < 2; r++) {
                    const uint32_t cs = low_s >= 0 ? scnt[low_s] : 0x80000000u;
                    const uint32_t cn = low_n < nn ? ncnt[low_n] : 0x40000000u;
                    if (cs < cn) { sum += cs; pleaf[low_s] = (uint8_t)nn; low_s--; }
                    else { sum += cn; pnode[low_n] = (uint8_t)nn; low_n++; }
                }
                ncnt[nn++] = sum;
            }
            const uint32_t root = nleaf - 2u;
            depth[root] = 0;
            for (int i = (int)root - 1; i >= 0; i--) depth[i] = (uint8_t)(depth[pnode[i]] + 1);
            for (uint32_t i = 0; i < nleaf; i++) nb[i] = (uint8_t)(depth[pleaf[i]] + 1);
            const uint32_t largest_bits = nb[last];
            const uint32_t max_nb = fse_optimal_table_log(table_log, n, max_sym, 1u);
            uint32_t tl = largest_bits;
            if (largest_bits > max_nb) {
                tl = max_nb;
                int total_cost = 0;
                const uint32_t base_cost = 1u << (largest_bits - max_nb);
                int m = (int)last;
                while (nb[m] > max_nb) { total_cost += (int)(base_cost - (1u << (largest_bits - nb[m]))); nb[m] = (uint8_t)max_nb; m--; }
                while (nb[m] == max_nb) m--;
                total_cost >>= (largest_bits - max_nb);
                constexpr uint32_t kNone = 0xF0F0F0F0u;
                for (int r = 0; r < 16; r++) rank_last[r] = kNone;
                {
                    uint32_t cur = max_nb;
                    for (int pos = m; pos >= 0; pos--) {
                        if (nb[pos] >= cur) continue;
                        cur = nb[pos];
                        rank_last[max_nb - cur] = (uint32_t)pos;
                    }
                }
                while (total_cost > 0) {
                    uint32_t dec = highbit32((uint32_t)total_cost) + 1u;
                    for (; dec > 1; dec--) {
                        const uint32_t hi = rank_last[dec], lo = rank_last[dec - 1];
                        if (hi == kNone) continue;
                        if (lo == kNone) break;
                        if (scnt[hi] <= 2u * scnt[lo]) break;
                    }
                    while (dec <= 12u && rank_last[dec] == kNone) dec++;
                    total_cost -= 1 << (dec - 1);
                    if (rank_last[dec - 1] == kNone) rank_last[dec - 1] = rank_last[dec];
                    nb[rank_last[dec]]++;
                    if (rank_last[dec] == 0) rank_last[dec] = kNone;
                    else {
                        rank_last[dec]--;
                        if (nb[rank_last[dec]] != max_nb - dec) rank_last[dec] = kNone;
                    }
                }
                while (total_cost < 0) {
                    if (rank_last[1] == kNone) {
                        while (nb[m] == max_nb) m--;
                        nb[m + 1]--;
                        rank_last[1] = (uint32_t)(m + 1);
                        total_cost++;
                        continue;
                    }
                    nb[rank_last[1] + 1]--;
                    rank_last[1]++;
                    total_cost++;
                }
            }
            for (int k = 0; k < 256; k++) lens[k] = 0;
            for (uint32_t i = 0; i < nleaf; i++) lens[ssym[i]] = nb[i];
            // ---- HUF_writeCTable: weights of symbols 0 .. max_sym - 1, FSE-coded (HUF_compressWeights) or 4-bit
            for (uint32_t k = 0; k < max_sym; k++) wts[k] = lens[k] ? (uint8_t)(tl + 1u - lens[k]) : (uint8_t)0;
            const uint32_t nw = max_sym;
            int hsize = 0;                                 // HUF_compressWeights' result (-1: an error, HUF_compress fails)
            if (nw > 1) {
                for (int k = 0; k < 16; k++) { wcnt[k] = 0; wnorm[k] = 0; }
                for (uint32_t k = 0; k < nw; k++) wcnt[wts[k]]++;
                uint32_t maxw = 0, maxc = 0;
                for (uint32_t k = 0; k <= 12; k++) { if (wcnt[k]) maxw = k; maxc = wcnt[k] > maxc ? wcnt[k] : maxc; }
                if (maxc == nw) hsize = 1;
                else if (maxc == 1) hsize = 0;
                else {
                    const uint32_t wtl = fse_optimal_table_log(6u, nw, maxw, 2u);
                    // FSE_normalizeCount, useLowProbCount = 0: low-probability weights get 1
                    const uint64_t scale = 62u - wtl, step = (1ull << 62) / nw, vstep = 1ull << (scale - 20u);
                    const uint32_t rtb[8] = {0, 473195, 504333, 520860, 550000, 700000, 750000, 830000};
                    int still = 1 << wtl;
                    uint32_t lg = 0;
                    int lgp = 0;
                    const uint32_t low_thr = nw >> wtl;
                    for (uint32_t k = 0; k <= maxw; k++) {
                        const uint32_t ck = wcnt[k];
                        if (ck == 0) { wnorm[k] = 0; continue; }
                        if (ck <= low_thr) { wnorm[k] = 1; still--; }
                        else {
                            int proba = (int)(((uint64_t)ck * step) >> scale);
                            if (proba < 8) {
                                const uint64_t rest = vstep * rtb[proba];
                                proba += ((uint64_t)ck * step) - ((uint64_t)proba << scale) > rest;
                            }
                            if (proba > lgp) { lgp = proba; lg = k; }
                            wnorm[k] = proba;
                            still -= proba;
                        }
                    }
                    bool ok = true;
                    if (-still >= (wnorm[lg] >> 1)) {
                        // FSE_normalizeM2
                        constexpr int kNA = -2;
                        uint32_t total = nw, distributed = 0;
                        uint32_t low_one = (uint32_t)(((uint64_t)nw * 3u) >> (wtl + 1u));
                        for (uint32_t k = 0; k <= maxw; k++) {
                            const uint32_t ck = wcnt[k];
                            if (ck == 0) { wnorm[k] = 0; continue; }
                            if (ck <= low_thr || ck <= low_one) { wnorm[k] = 1; distributed++; total -= ck; continue; }
                            wnorm[k] = kNA;
                        }
                        uint32_t to_dist = (1u << wtl) - distributed;
                        if (to_dist != 0) {
                            if (total / to_dist > low_one) {
                                low_one = (uint32_t)(((uint64_t)total * 3u) / ((uint64_t)to_dist * 2u));
                                for (uint32_t k = 0; k <= maxw; k++)
                                    if (wnorm[k] == kNA && wcnt[k] <= low_one) { wnorm[k] = 1; distributed++; total -= wcnt[k]; }
                                to_dist = (1u << wtl) - distributed;
                            }
                            if (distributed == maxw + 1u) {
                                uint32_t mv = 0, mc = 0;
                                for (uint32_t k = 0; k <= maxw; k++) if (wcnt[k] > mc) { mv = k; mc = wcnt[k]; }
                                wnorm[mv] += (int)to_dist;
                            } else if (total == 0) {
                                for (uint32_t k = 0; to_dist > 0; k = (k + 1u) % (maxw + 1u))
                                    if (wnorm[k] > 0) { to_dist--; wnorm[k]++; }
                            } else {
                                const uint32_t vlog = 62u - wtl;
                                const uint64_t mid = (1ull << (vlog - 1u)) - 1u;
                                const uint64_t rstep = (((1ull << vlog) * to_dist) + mid) / total;
                                uint64_t tmp = mid;
                                for (uint32_t k = 0; k <= maxw; k++)
                                    if (wnorm[k] == kNA) {
                                        const uint64_t end = tmp + (uint64_t)wcnt[k] * rstep;
                                        const uint32_t wgt = (uint32_t)(end >> vlog) - (uint32_t)(tmp >> vlog);
                                        if (wgt < 1) ok = false;
                                        wnorm[k] = (int)wgt;
                                        tmp = end;
                                    }
                            }
                        }
                    } else wnorm[lg] += still;
                    // FSE_writeNCount into hdr + 1
                    BitW bw{hdr + 1, 0, 0, 0};
                    if (ok) {
                        bw.add(wtl - 5u, 4);
                        int remaining = (1 << wtl) + 1, threshold = 1 << wtl, nbits = (int)wtl + 1;
                        bool prev0 = false;
                        uint32_t sym = 0;
                        while (sym <= maxw && remaining > 1) {
                            if (prev0) {
                                uint32_t start = sym;
                                while (sym <= maxw && !wnorm[sym]) sym++;
                                if (sym > maxw) break;
                                while (sym >= start + 24) { start += 24; bw.add(0xFFFFu, 16); }
                                while (sym >= start + 3) { start += 3; bw.add(3, 2); }
                                bw.add(sym - start, 2);
                            }
                            int cc = wnorm[sym++];
                            const int mx = (2 * threshold - 1) - remaining;
                            remaining -= cc < 0 ? -cc : cc;
                            cc++;
                            if (cc >= threshold) cc += mx;
                            bw.add((uint32_t)cc, nbits - (cc < mx));
                            prev0 = cc == 1;
                            if (remaining < 1) { ok = false; break; }
                            while (remaining < threshold) { nbits--; threshold >>= 1; }
                        }
                        if (remaining != 1) ok = false;
                    }
                    if (!ok) hsize = -1;
                    else if (nw <= 2) { bw.close(false); hsize = 0; }                 // FSE_compress_usingCTable: nothing below 3 symbols
                    else {
                        bw.close(false);
                        const uint32_t hb = bw.n;
                        // FSE_buildCTable: spread (step 5/8 size + 3, no low-probability cells: useLowProbCount = 0), state table
                        const uint32_t size = 1u << wtl, mask = size - 1u, stp = (size >> 1) + (size >> 3) + 3u;
                        uint32_t pos = 0;
                        for (uint32_t k = 0; k <= maxw; k++)
                            for (int o = 0; o < wnorm[k]; o++) { tsym[pos] = (uint8_t)k; pos = (pos + stp) & mask; }
                        uint32_t cum[14];
                        cum[0] = 0;
                        for (uint32_t k = 1; k <= maxw + 1u; k++) cum[k] = cum[k - 1] + (uint32_t)wnorm[k - 1];
                        for (uint32_t u = 0; u < size; u++) stab[cum[tsym[u]]++] = (uint16_t)(size + u);
                        int dnb[13], dfs[13];
                        int total = 0;
                        for (uint32_t k = 0; k <= maxw; k++) {
                            const int nk = wnorm[k];
                            if (nk == 0) { dnb[k] = (int)(((wtl + 1u) << 16) - size); dfs[k] = 0; }
                            else if (nk == 1) { dnb[k] = (int)((wtl << 16) - size); dfs[k] = total - 1; total += 1; }
                            else {
                                const uint32_t mbo = wtl - highbit32((uint32_t)nk - 1u);
                                dnb[k] = (int)((mbo << 16) - ((uint32_t)nk << mbo));
                                dfs[k] = total - nk;
                                total += nk;
                            }
                        }
                        auto init = [&](uint32_t sy) -> uint32_t {
                            const uint32_t nbo = (uint32_t)(dnb[sy] + (1 << 15)) >> 16;
                            const uint32_t v = (nbo << 16) - (uint32_t)dnb[sy];
                            return stab[(int)(v >> nbo) + dfs[sy]];
                        };
                        BitW fw{hdr + 1 + hb, 0, 0, 0};
                        auto enc = [&](uint32_t st, uint32_t sy) -> uint32_t {
                            const uint32_t nbo = (st + (uint32_t)dnb[sy]) >> 16;
                            fw.add(st & ((1u << nbo) - 1u), (int)nbo);
                            return stab[(int)(st >> nbo) + dfs[sy]];
                        };
                        int i = (int)nw;
                        uint32_t s1, s2;
                        if (nw & 1u) { s1 = init(wts[i - 1]); s2 = init(wts[i - 2]); i -= 2; s1 = enc(s1, wts[i - 1]); i--; }
                        else { s2 = init(wts[i - 1]); s1 = init(wts[i - 2]); i -= 2; }
                        while (i > 0) { s2 = enc(s2, wts[i - 1]); s1 = enc(s1, wts[i - 2]); i -= 2; }
                        fw.add(s2 & mask, (int)wtl);
                        fw.add(s1 & mask, (int)wtl);
                        hsize = (int)(hb + fw.close(true));
                    }
                }
            }
            uint32_t hlen = 0;
            bool fail = hsize < 0;
            if (!fail) {
                if (hsize > 1 && hsize < (int)(max_sym / 2u)) { hdr[0] = (uint8_t)hsize; hlen = (uint32_t)hsize + 1u; }
                else if (max_sym > 128u) fail = true;
                else {
                    hdr[0] = (uint8_t)(127u + max_sym);
                    for (uint32_t k = 0; k < max_sym; k += 2)
                        hdr[1 + k / 2] = (uint8_t)((wts[k] << 4) | (k + 1 < max_sym ? wts[k + 1] : 0u));
                    hlen = (max_sym + 1u) / 2u + 1u;
                }
            }
            if (fail || hlen + 12u >= n) hlen = 0;
            // canonical code values (HUF_buildCTable): per length ascending symbols, the longest codes lowest
            if (hlen) {
                uint32_t per[16], start[16];
                for (int l = 0; l < 16; l++) { per[l] = 0; start[l] = 0; }
                for (int k = 0; k <= (int)max_sym; k++) per[lens[k]]++;
                uint32_t mn = 0;
                for (uint32_t l = tl; l > 0; l--) { start[l] = mn; mn += per[l]; mn >>= 1; }
                for (int k = 0; k < 256; k++) code[k] = lens[k] ? (uint16_t)(start[lens[k]]++ | ((uint32_t)lens[k] << 12)) : (uint16_t)0;
            }
            s_hlen = hlen;
            s_tl = tl;
        }
        __syncthreads();
        if (s_hlen == 0) mode = 1;
    }
    // ---- the four streams' byte counts (bits + the closing 1 bit) from the per-stream histograms
    uint32_t bytes[4] = {0, 0, 0, 0};
    const uint32_t hlen = mode == 3 ? s_hlen : 0u;
    if (mode == 3) {
        for (int j = 0; j < 4; j++) {
            uint32_t b = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) b += hist[j][4 * t + e] * (uint32_t)(code[4 * t + e] >> 12);
            bytes[j] = (wave_sum32(b) + 1u + 7u) >> 3;
        }
        if ((uint64_t)hlen + 6u + bytes[0] + bytes[1] + bytes[2] + bytes[3] >= (uint64_t)n - 1u) mode = 1;
    }
    if (mode == 3) {
        for (int k = t; k < 128; k += 64) rec[kXRecHdr + k] = k < (int)hlen ? hdr[k] : (uint8_t)0;
        for (int k = t; k < 256; k += 64) ((uint16_t*)(rec + kXRecTab))[k] = code[k];
    }
    if (t == 0) {
        ((uint32_t*)rec)[0] = mode == 3 ? hlen : 0u;
        ((uint32_t*)rec)[1] = mode == 3 ? s_tl : 0u;
        bsizes[c] = mode == 0 ? 0u : mode == 1 ? n : mode == 2 ? 1u : hlen + 6u + bytes[0] + bytes[1] + bytes[2] + bytes[3];
        meta[c] = (uint64_t)bytes[0] | ((uint64_t)bytes[1] << 16) | ((uint64_t)bytes[2] << 32) | ((uint64_t)mode << 48);
    }
}

// X2.  A wave = 16 chunks x 4 streams, each chunk's code table in LDS (16 KB a wave).
constexpr int kXChunksPerWave = 16;
__global__ void __launch_bounds__(64) huf0x_encode_kernel(const uint8_t* __restrict__ dense, const uint64_t* __restrict__ offsets,
                                                          const uint32_t* __restrict__ sizes, uint64_t nchunks,
                                                          const uint8_t* __restrict__ recs, const uint64_t* __restrict__ meta,
                                                          uint8_t* __restrict__ out, const uint64_t* __restrict__ boffs)
{
    __shared__ uint32_t tab[kXChunksPerWave][256];     // value | length << 16
    const int t = threadIdx.x, j = t & 3, ci = t >> 2;
    const uint64_t c0 = (uint64_t)blockIdx.x * kXChunksPerWave;
    for (int k = 0; k < kXChunksPerWave; k++) {
        const uint64_t ck = c0 + (uint64_t)k;
        if (ck >= nchunks) break;
        const uint16_t* const ct = (const uint16_t*)(recs + ck * kXRecBytes + kXRecTab);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t v = ct[4 * t + e];
            tab[k][4 * t + e] = (v & 0xfffu) | ((v >> 12) << 16);
        }
    }
    __syncthreads();
    const uint64_t c = c0 + (uint64_t)ci;
    if (c >= nchunks) return;
    const uint32_t n = sizes[c];
    const uint8_t* const s = dense + offsets[c];
    uint8_t* const o = out + boffs[c];
    const uint64_t m = meta[c];
    const uint32_t mode = (uint32_t)(m >> 48);
    if (mode == 0) return;
    if (mode == 2) { if (j == 0) o[0] = s[0]; return; }
    if (mode == 1) {                                      // stored: 16-byte pieces over the quad, then the odd bytes
        uint32_t k = (uint32_t)j * 16u;
        for (; k + 16 <= n; k += 64) *(u32x4_a1*)(o + k) = *(const u32x4_a1*)(s + k);
        for (uint32_t r = (n & ~15u) + (uint32_t)j; r < n; r += 4) o[r] = s[r];
        return;
    }
    const uint8_t* const rec = recs + c * kXRecBytes;
    const uint32_t hlen = ((const uint32_t*)rec)[0];
    const uint32_t b0 = (uint32_t)(m & 0xffffu), b1 = (uint32_t)((m >> 16) & 0xffffu), b2 = (uint32_t)((m >> 32) & 0xffffu);
    for (uint32_t k = (uint32_t)j; k < hlen; k += 4) o[k] = rec[kXRecHdr + k];
    if (j == 0) {
        uint8_t* const jt = o + hlen;
        jt[0] = (uint8_t)b0; jt[1] = (uint8_t)(b0 >> 8); jt[2] = (uint8_t)b1; jt[3] = (uint8_t)(b1 >> 8); jt[4] = (uint8_t)b2; jt[5] = (uint8_t)(b2 >> 8);
    }
    uint8_t* const so = o + hlen + 6 + (j > 0 ? b0 : 0u) + (j > 1 ? b1 : 0u) + (j > 2 ? b2 : 0u);
    uint32_t k0, k1;
    sub_range(n, j, k0, k1);
    if (j == 3) k1 = n;
    const uint32_t* const tb = tab[ci];
    uint64_t acc = 0;
    uint32_t nbits = 0, wd = 0;                           // dwords written
    auto put = [&](uint32_t sym) {
        const uint32_t e = tb[sym];
        acc |= (uint64_t)(e & 0xffffu) << nbits;
        nbits += e >> 16;
        if (nbits >= 32) { *(u32_any*)(so + 4u * wd) = (uint32_t)acc; wd++; acc >>= 32; nbits -= 32; }
    };
    // last symbol first: the ragged end byte by byte, then 16 source bytes a load
    uint32_t k = k1;
    const uint32_t r = (k1 - k0) & 15u;
    for (uint32_t i = 0; i < r; i++) put(s[--k]);
    while (k > k0) {
        k -= 16;
        const u32x4 x = *(const u32x4_a1*)(s + k);
#pragma unroll
        for (int d = 3; d >= 0; d--) {
            const uint32_t v = d == 0 ? x.x : d == 1 ? x.y : d == 2 ? x.z : x.w;
            put(v >> 24); put((v >> 16) & 255u); put((v >> 8) & 255u); put(v & 255u);
        }
    }
    acc |= 1ull << nbits;                                 // the closing 1 bit (BIT_closeCStream)
    nbits += 1;
    if (nbits >= 32) { *(u32_any*)(so + 4u * wd) = (uint32_t)acc; wd++; acc >>= 32; nbits -= 32; }
    uint8_t* tail = so + 4u * wd;
    for (uint32_t b = 0; b < nbits; b += 8) *tail++ = (uint8_t)(acc >> b);
}
