// zone_probe.cpp -- the rules of zone-map pruning (sprintz_amd/csrc/zone.h) on a host compiler, for tests/test_zone_cpu.py.  One query
// per line on stdin, whitespace-separated integers behind a keyword, and one answer per line:
//     box  esz D chunk_len zlen too_wide mode  zmin[D] zmax[D] lo[D] hi[D]      -> the chunk's class (0 NONE, 1 ALL, 2 DECODE)
//     lin  esz D chunk_len zlen too_wide bias lo hi  w[D] zmin[D] zmax[D]       -> the chunk's class
//     span first_offset end_offset                                               -> 1 if the container is too wide to prune, else 0
//     rows zlen chunk_len D                                                      -> the chunk's existing rows
//     byte rows j                                                                -> mask byte j of a chunk whose `rows` rows all match
//     tmp  nchunks                                                               -> bytes of the flags in front of the scan's scratch
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "../sprintz_amd/csrc/zone.h"

using namespace sprintz;

template <typename T>
static std::vector<T> take(std::istringstream& in, uint32_t D)
{
    std::vector<T> v(D);
    for (uint32_t d = 0; d < D; d++) {
        long long x = 0;
        in >> x;
        v[d] = (T)x;
    }
    return v;
}

template <typename T>
static int box(std::istringstream& in, uint32_t D, uint32_t chunk_len, int64_t zlen, bool wide, uint32_t mode)
{
    const auto zmin = take<T>(in, D), zmax = take<T>(in, D), lo = take<T>(in, D), hi = take<T>(in, D);
    return zone_classify_box<T>(zlen, chunk_len, D, wide, zmin.data(), zmax.data(), lo.data(), hi.data(), mode);
}

template <typename T>
static int lin(std::istringstream& in, uint32_t D, uint32_t chunk_len, int64_t zlen, bool wide, int32_t bias, int32_t lo, int32_t hi)
{
    const auto w = take<int32_t>(in, D);
    const auto zmin = take<T>(in, D), zmax = take<T>(in, D);
    return zone_classify_linear<T>(zlen, chunk_len, D, wide, zmin.data(), zmax.data(), w.data(), bias, lo, hi);
}

int main()
{
    static_assert(kZoneSpanLimit == 0xf0000000ull, "the span rule's constant");
    static_assert(zone_all_mask_byte(3, 0) == 7 && zone_all_mask_byte(8, 0) == 0xff && zone_all_mask_byte(8, 1) == 0, "constexpr rules");
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string key;
        if (!(in >> key)) continue;
        if (key == "box" || key == "lin") {
            long long esz, D, chunk_len, zlen, wide;
            in >> esz >> D >> chunk_len >> zlen >> wide;
            if ((esz != 1 && esz != 2) || D < 1 || D > 512) { printf("bad query\n"); return 2; }
            if (key == "box") {
                long long mode;
                in >> mode;
                printf("%d\n", esz == 1 ? box<uint8_t>(in, (uint32_t)D, (uint32_t)chunk_len, zlen, wide != 0, (uint32_t)mode)
                                        : box<uint16_t>(in, (uint32_t)D, (uint32_t)chunk_len, zlen, wide != 0, (uint32_t)mode));
            } else {
                long long bias, lo, hi;
                in >> bias >> lo >> hi;
                printf("%d\n", esz == 1 ? lin<uint8_t>(in, (uint32_t)D, (uint32_t)chunk_len, zlen, wide != 0, (int32_t)bias, (int32_t)lo, (int32_t)hi)
                                        : lin<uint16_t>(in, (uint32_t)D, (uint32_t)chunk_len, zlen, wide != 0, (int32_t)bias, (int32_t)lo, (int32_t)hi));
            }
        } else if (key == "span") {
            unsigned long long a, b;
            in >> a >> b;
            printf("%d\n", zone_span_too_wide(a, b) ? 1 : 0);
        } else if (key == "rows") {
            long long zlen, chunk_len, D;
            in >> zlen >> chunk_len >> D;
            printf("%u\n", zone_rows(zlen, (uint32_t)chunk_len, (uint32_t)D));
        } else if (key == "byte") {
            unsigned long long rows, j;
            in >> rows >> j;
            printf("%u\n", (unsigned)zone_all_mask_byte((uint32_t)rows, (uint32_t)j));
        } else if (key == "tmp") {
            unsigned long long n;
            in >> n;
            printf("%llu\n", (unsigned long long)zone_flags_bytes(n));
        } else {
            printf("bad key %s\n", key.c_str());
            return 2;
        }
    }
    return 0;
}
