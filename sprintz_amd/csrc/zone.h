// zone.h -- the rules of zone-map pruning, host and kernels alike: a chunk's class under a box or a linear predicate from its per-column
// minimum and maximum, the span from which a container is not pruned, the scratch of a prune call and the mask bytes expand writes for a
// chunk it did not decode.  Plain C++17, no HIP, constexpr throughout: zone.hip's kernels call these, and a host compiler builds them
// (tests/zone_probe.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

namespace sprintz {

// a chunk's class under one predicate: no row matches / every existing row matches / the decoder must look
constexpr uint8_t kZoneNone = 0, kZoneAll = 1, kZoneDecode = 2;
constexpr uint32_t kZoneFilterAll = 0, kZoneFilterAny = 1;      // SPRINTZ_FILTER_ALL / SPRINTZ_FILTER_ANY

// The 4 GiB rule.  decode_fast.h and decode_uni.h address the streams of one wavefront as 32-bit offsets from the wavefront's first
// stream; in a container as compress_batch_dense builds it the chunks of a wavefront lie side by side, but compaction puts any two
// chunks of the batch into one.  A container that spans this much or more is therefore not pruned: every chunk is kZoneDecode.
constexpr uint64_t kZoneSpanLimit = 0xf0000000ull;
constexpr bool zone_span_too_wide(uint64_t first_offset, uint64_t end_offset) { return end_offset - first_offset >= kZoneSpanLimit; }

// existing rows of a chunk whose decoder returned zlen >= 0 elements (a partial last row is not a row; never more than the slot holds)
constexpr uint32_t zone_rows(int64_t zlen, uint32_t chunk_len, uint32_t D)
{
    const uint64_t r = (uint64_t)zlen / D, cap = chunk_len / D;
    return (uint32_t)(r < cap ? r : cap);
}

// what the element count alone decides: a damaged chunk stays among the survivors (expand reports it with the map's code, whatever the
// decoder makes of it: a truncated stream is told by its length, which compaction stretches); a chunk without a
// row matches nothing; -1: the bounds decide
constexpr int zone_class_by_len(int64_t zlen, uint32_t chunk_len, uint32_t D, bool too_wide)
{
    return (zlen < 0 || too_wide) ? (int)kZoneDecode : zone_rows(zlen, chunk_len, D) == 0 ? (int)kZoneNone : -1;
}

// ---- box (filter_rows): unsigned, inclusive.  One column's verdict as bits: 1 = disjoint (no value of the column can match),
// 2 = inside (every value does).  The columns fold with OR into `some` and with AND into `every` (start: 0 and 3).
constexpr uint32_t kZoneDisjoint = 1, kZoneInside = 2;
template <typename T>
constexpr uint32_t zone_box_column(T zmin, T zmax, T lo, T hi)
{
    return ((lo > hi || zmax < lo || zmin > hi) ? kZoneDisjoint : 0u) | ((lo <= zmin && zmax <= hi) ? kZoneInside : 0u);
}
constexpr uint8_t zone_box_class(uint32_t some, uint32_t every, uint32_t mode)
{
    if (mode == kZoneFilterAll) return (some & kZoneDisjoint) ? kZoneNone : (every & kZoneInside) ? kZoneAll : kZoneDecode;
    return (some & kZoneInside) ? kZoneAll : (every & kZoneDisjoint) ? kZoneNone : kZoneDecode;
}

// ---- linear form (filter_linear without a lag term): bias + sum_d w[d] x[d] over a chunk's rows lies in [smin, smax], both exact in
// int64 (|w| < 2^31, x < 2^16, at most 512 columns: below 2^57).  A column adds its term to each end.
constexpr int64_t zone_linear_min_term(int32_t w, uint32_t zmin, uint32_t zmax) { return (int64_t)w * (int64_t)(w >= 0 ? zmin : zmax); }
constexpr int64_t zone_linear_max_term(int32_t w, uint32_t zmin, uint32_t zmax) { return (int64_t)w * (int64_t)(w >= 0 ? zmax : zmin); }
// a range that leaves int32 is the decoder's: the kernel's 32-bit sum may wrap there, and only the decoder knows what it yields
constexpr uint8_t zone_linear_class(int64_t smin, int64_t smax, int32_t lo, int32_t hi)
{
    if (smin < (int64_t)INT32_MIN || smax > (int64_t)INT32_MAX) return kZoneDecode;
    if (lo > hi || smax < (int64_t)lo || smin > (int64_t)hi) return kZoneNone;
    return ((int64_t)lo <= smin && smax <= (int64_t)hi) ? kZoneAll : kZoneDecode;
}

// ---- a whole chunk, one column after the other (the kernels fold the same pieces over a lane group)
template <typename T>
constexpr uint8_t zone_classify_box(int64_t zlen, uint32_t chunk_len, uint32_t D, bool too_wide, const T* zmin, const T* zmax, const T* lo,
                                    const T* hi, uint32_t mode)
{
    const int by_len = zone_class_by_len(zlen, chunk_len, D, too_wide);
    if (by_len >= 0) return (uint8_t)by_len;
    uint32_t some = 0, every = kZoneDisjoint | kZoneInside;
    for (uint32_t d = 0; d < D; d++) {
        const uint32_t v = zone_box_column(zmin[d], zmax[d], lo[d], hi[d]);
        some |= v;
        every &= v;
    }
    return zone_box_class(some, every, mode);
}
template <typename T>
constexpr uint8_t zone_classify_linear(int64_t zlen, uint32_t chunk_len, uint32_t D, bool too_wide, const T* zmin, const T* zmax,
                                       const int32_t* w, int32_t bias, int32_t lo, int32_t hi)
{
    const int by_len = zone_class_by_len(zlen, chunk_len, D, too_wide);
    if (by_len >= 0) return (uint8_t)by_len;
    int64_t smin = bias, smax = bias;
    for (uint32_t d = 0; d < D; d++) {
        smin += zone_linear_min_term(w[d], zmin[d], zmax[d]);
        smax += zone_linear_max_term(w[d], zmin[d], zmax[d]);
    }
    return zone_linear_class(smin, smax, lo, hi);
}

// ---- expand: mask byte j of a chunk every one of whose `rows` existing rows matches -- rows 8 j .. 8 j + 7 below `rows` set, the
// rest (the padding bits of the last byte among them) 0
constexpr uint8_t zone_all_mask_byte(uint32_t rows, uint32_t j)
{
    const uint64_t first = 8ull * j;
    return rows >= first + 8 ? (uint8_t)0xff : rows > first ? (uint8_t)((1u << (rows - (uint32_t)first)) - 1u) : (uint8_t)0;
}

// ---- scratch of one prune call: a u32 flag a chunk (is it kZoneDecode?) in front of the size scan's own scratch, which starts on 8 bytes
constexpr size_t zone_flags_bytes(uint64_t nchunks) { return (size_t)((nchunks * 4 + 7) & ~7ull); }

}  // namespace sprintz
