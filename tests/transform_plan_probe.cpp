// transform_plan_probe.cpp -- the stand-alone transforms' decode plan (sprintz_amd/csrc/transform_plan.h) on a host compiler, for
// tests/test_transform_plan_cpu.py: that this file builds with g++ is itself the check that the header holds no HIP.  Reads one query per
// line from stdin,
//     plan  kind=0|1 esz=1|2 len=N D=N src_lo=N dst_lo=N chain=-1|0|N cus=N      (what is not named keeps its default)
// chain being SPRINTZ_MI355X_TRANSFORM_CHAIN as the library reads it (-1: not set), and prints the plan, the scratch size the library
// reports for the shape, the size the library reported BEFORE the two were derived from one description (`parent`: one summary per 16
// rows + the one-pass decode's slack) with what its launcher took then (`parent_used`), and every array of the call as
// name:offset:bytes.  `sweep` runs the property sweep of the module's docstring inside the probe and prints one line per violation, then
// the number of cases.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../sprintz_amd/csrc/transform_plan.h"

using namespace sprintz;

static const char* family_name(int f) { return f == SPRINTZ_KF_TR_CHAIN ? "tr_chain" : f == SPRINTZ_KF_TR_WAVE ? "tr_wave" : f == SPRINTZ_KF_TR_LEVELS ? "tr_levels" : "none"; }

static uint64_t chain_min_of(long long setting) { return setting < 0 ? (uint64_t)TR_CHAIN_MIN_TILES : setting == 0 ? kTrChainNever : (uint64_t)setting; }

// what sprintz_mi355x_transform_tmp_bytes returned before: the generic levels' layout for every form, + 8 KiB + len / 8 + 64
static uint64_t parent_tmp_bytes(int kind, int esz, uint64_t len, uint32_t D)
{
    uint64_t rows = (len + D - 1) / D, total = 0;
    while (rows > 1) {
        rows = (rows + 15) / 16;
        total += ((rows * D * (uint64_t)esz + 63) & ~(uint64_t)63) * (kind ? 4 : 2);
    }
    return total + len * (uint64_t)esz / 8 + 8192 + 64;
}

// what the launcher took from d_tmp before: today's arrays + the generic levels' top level, which it placed (a single run: one row of the
// levels' D elements, two or four times) and reduced into although nothing read it
static uint64_t parent_used(const TrShape& s, const TrPlan& p)
{
    const bool top_level = p.nlevels > 0 && p.top != kTrTopRuns && p.lv[p.nlevels - 1].s1 == kTrNone;
    return p.used + (top_level ? (((uint64_t)p.D * s.esz + 63) & ~(uint64_t)63) * (s.kind ? 4 : 2) : 0);
}

struct Arr { const char* name; uint64_t off, bytes; };
static std::vector<Arr> arrays_of(const TrPlan& p)
{
    std::vector<Arr> a;
    tr_arrays(p, [&](const char* name, uint64_t off, uint64_t bytes) { a.push_back(Arr{name, off, bytes}); });
    return a;
}

static std::string show(const TrShape& s, const TrPlan& p)
{
    char b[512];
    std::string out;
    snprintf(b, sizeof b, "family=%s piece=%d M=%d D=%u dv=%u len_e=%llu rows0=%llu run_loads=%d run_rows=%llu nruns=%llu grid=%llu top=%s G=%u nlevels=%d",
             family_name(p.family), p.piece, p.M, p.D, p.dv, (unsigned long long)p.len_e, (unsigned long long)p.rows0, p.run_loads, (unsigned long long)p.run_rows,
             (unsigned long long)p.nruns, (unsigned long long)p.grid, p.top == kTrTopRuns ? "runs" : p.top == kTrTopLevels ? "levels" : "none", p.G, p.nlevels);
    out = b;
    snprintf(b, sizeof b, " tile_e=%llu ntiles=%llu wgs=%llu need=%llu used=%llu tmp_bytes=%llu parent=%llu parent_used=%llu", (unsigned long long)p.tile_e, (unsigned long long)p.ntiles,
             (unsigned long long)p.wgs, (unsigned long long)p.need, (unsigned long long)p.used, (unsigned long long)tr_tmp_bytes(s.kind, s.esz, s.len, s.D),
             (unsigned long long)parent_tmp_bytes(s.kind, s.esz, s.len, s.D), (unsigned long long)parent_used(s, p));
    out += b;
    out += " levels=";
    for (int k = 0; k < p.nlevels; k++) {
        snprintf(b, sizeof b, "%s%llu:%llu", k ? "," : "", (unsigned long long)p.lv[k].rows, (unsigned long long)p.lv[k].span);
        out += b;
    }
    out += " arrays=";
    bool first = true;
    for (const Arr& a : arrays_of(p)) {
        snprintf(b, sizeof b, "%s%s:%llu:%llu", first ? "" : ",", a.name, (unsigned long long)a.off, (unsigned long long)a.bytes);
        out += b;
        first = false;
    }
    return out;
}

static bool same_level(const TrLevel& a, const TrLevel& b)
{
    return a.rows == b.rows && a.span == b.span && a.bytes == b.bytes && a.s1 == b.s1 && a.s2 == b.s2 && a.xin == b.xin && a.din == b.din;
}
static bool same(const TrPlan& a, const TrPlan& b)
{
    if (!(a.family == b.family && a.piece == b.piece && a.M == b.M && a.D == b.D && a.dv == b.dv && a.len_e == b.len_e && a.rows0 == b.rows0 &&
          a.run_loads == b.run_loads && a.run_rows == b.run_rows && a.nruns == b.nruns && a.grid == b.grid && a.top == b.top && a.G == b.G &&
          a.nlevels == b.nlevels && a.tile_e == b.tile_e && a.ntiles == b.ntiles && a.arr == b.arr && a.need == b.need && a.wgs == b.wgs &&
          a.ticket == b.ticket && a.agg1 == b.agg1 && a.inc1 == b.inc1 && a.agg2 == b.agg2 && a.inc2 == b.inc2 && a.used == b.used))
        return false;
    for (int k = 0; k < a.nlevels; k++)
        if (!same_level(a.lv[k], b.lv[k])) return false;
    return true;
}

static unsigned long long g_bad = 0;
static void bad(const char* what, const TrShape& s, long long chain, const TrPlan& p)
{
    if (++g_bad > 200) return;
    printf("violation: %s: kind=%d esz=%d len=%llu D=%u src_lo=%u dst_lo=%u chain=%lld -> %s\n", what, s.kind, s.esz, (unsigned long long)s.len, s.D, s.src_lo, s.dst_lo,
           chain, show(s, p).c_str());
}

// one case of the sweep: the properties of the module's docstring, against the size reported for the shape
static void check_case(const TrShape& s, long long chain, uint64_t tmp_bytes)
{
    const TrPlan p = tr_plan(s);
    if (!same(p, tr_plan(s))) bad("another answer the second time", s, chain, p);
    // exactly one form, and only that form's arrays
    const bool chain_f = p.family == SPRINTZ_KF_TR_CHAIN, wave_f = p.family == SPRINTZ_KF_TR_WAVE, levels_f = p.family == SPRINTZ_KF_TR_LEVELS;
    if ((int)chain_f + (int)wave_f + (int)levels_f != 1) bad("not exactly one form", s, chain, p);
    if (chain_f && !(p.piece == 16 && s.esz == 2 && p.ntiles >= 1 && p.ticket == 0 && p.nlevels == 0 && p.top == kTrTopNone && p.wgs >= 1 && p.wgs <= s.cus && p.need <= tmp_bytes))
        bad("the one-pass form with another form's parts", s, chain, p);
    if (wave_f && !(p.piece != 0 && p.ticket == kTrNone && p.ntiles == 0 && p.nruns >= 1 && (p.nruns == 1) == (p.nlevels == 0) && (p.top == kTrTopNone) == (p.nruns == 1) &&
                    (p.top != kTrTopRuns || (p.nlevels == 1 && p.G >= 1 && p.G * p.D <= (uint32_t)kTrTopT)) && p.dv >= 1 && p.dv <= 64 && p.grid >= 1 && p.grid <= 0x7fffffffull))
        bad("the wave form with another form's parts", s, chain, p);
    if (levels_f && !(p.piece == 0 && p.ticket == kTrNone && p.ntiles == 0 && p.top == kTrTopNone && (p.nlevels == 0) == (p.rows0 <= 1)))
        bad("the generic levels with another form's parts", s, chain, p);
    if (p.nlevels > 0 && p.top != kTrTopRuns && (p.lv[p.nlevels - 1].rows != 1 || p.lv[p.nlevels - 1].s1 != kTrNone)) bad("the top level is not a single run without arrays", s, chain, p);
    for (int k = 0; k + 1 < p.nlevels; k++)
        if (p.lv[k].s1 == kTrNone || p.lv[k].xin == kTrNone || (s.kind != 0) != (p.lv[k].s2 != kTrNone) || (s.kind != 0) != (p.lv[k].din != kTrNone)) bad("a level below the top without its arrays", s, chain, p);
    // every array inside [0, tmp_bytes), no two overlapping (they are all live together)
    uint64_t end = 0;
    bool ordered = true;
    const std::vector<Arr> a = arrays_of(p);
    for (const Arr& x : a) {
        if (x.off == kTrNone || x.off + x.bytes > tmp_bytes || x.off + x.bytes > p.used) bad("an array outside [0, tmp_bytes) or past `used`", s, chain, p);
        ordered = ordered && x.off >= end;
        end = x.off + x.bytes;
    }
    if (!ordered)
        for (size_t i = 0; i < a.size(); i++)
            for (size_t j = i + 1; j < a.size(); j++)
                if (a[i].off < a[j].off + a[j].bytes && a[j].off < a[i].off + a[i].bytes && a[i].bytes && a[j].bytes) bad("two arrays overlap", s, chain, p);
    if (p.used > tmp_bytes) bad("more scratch used than reported", s, chain, p);
}

static void sweep()
{
    unsigned long long cases = 0, shapes = 0;
    const uint64_t rows_of[] = {1, 2, 5, 16, 17, 64, 65, 200, 256, 257, 1000, 4097, 16384, 16385, 70001};
    const uint64_t extras[] = {0, 1, 3};
    const unsigned los[] = {0, 1, 2, 4, 8};
    const long long chains[] = {-1, 0, 1};
    double worst = 0;
    for (int esz = 1; esz <= 2; esz++)
        for (int kind = 0; kind <= 1; kind++)
            for (uint32_t i = 1; i <= 1102; i++) {
                const uint32_t D = i <= 1100 ? i : i == 1101 ? 2047u : 65535u;
                for (uint64_t rows : rows_of)
                    for (uint64_t extra : extras) {
                        const uint64_t len = rows * D + extra, stream = len * esz;
                        const uint64_t tmp_bytes = tr_tmp_bytes(kind, esz, len, D);
                        shapes++;
                        // the cap: the size is not "twice the stream" -- the wave form's own use peaks at 1.07 x the stream, the one-pass decode's bound adds 0.125 x
                        if (tmp_bytes > stream + stream / 4 + 65536 || tmp_bytes != tr_tmp_bytes(kind, esz, len, D)) {
                            TrShape s; s.kind = kind; s.esz = esz; s.len = len; s.D = D;
                            bad("tmp_bytes above 1.25 x stream + 64 KiB, or another size the second time", s, -1, tr_plan(s));
                        }
                        if (stream > (1u << 20) && (double)tmp_bytes / (double)stream > worst) worst = (double)tmp_bytes / (double)stream;
                        for (unsigned src_lo : los)
                            for (unsigned dst_lo : los) {
                                if (esz == 2 && ((src_lo | dst_lo) & 1u)) continue;       // (odd addresses: uint8 only)
                                for (long long chain : chains) {
                                    TrShape s;
                                    s.kind = kind; s.esz = esz; s.len = len; s.D = D; s.src_lo = src_lo; s.dst_lo = dst_lo; s.chain_min = chain_min_of(chain);
                                    check_case(s, chain, tmp_bytes);
                                    cases++;
                                }
                            }
                    }
            }
    printf("sweep shapes=%llu cases=%llu violations=%llu worst_ratio_above_1MiB=%.4f\n", shapes, cases, g_bad, worst);
}

int main()
{
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string op, tok;
        if (!(in >> op)) continue;
        if (op == "sweep") { sweep(); continue; }
        if (op != "plan") { printf("bad op %s\n", op.c_str()); return 2; }
        TrShape s;
        long long chain = -1;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { printf("bad token %s\n", tok.c_str()); return 2; }
            const std::string key = tok.substr(0, eq);
            const long long v = strtoll(tok.c_str() + eq + 1, nullptr, 0);
            if (key == "kind") s.kind = (int)v;
            else if (key == "esz") s.esz = (int)v;
            else if (key == "len") s.len = (uint64_t)v;
            else if (key == "D") s.D = (uint32_t)v;
            else if (key == "src_lo") s.src_lo = (unsigned)v;
            else if (key == "dst_lo") s.dst_lo = (unsigned)v;
            else if (key == "chain") chain = v;
            else if (key == "cus") s.cus = (uint32_t)v;
            else { printf("bad token %s\n", tok.c_str()); return 2; }
        }
        s.chain_min = chain_min_of(chain);
        puts(show(s, tr_plan(s)).c_str());
    }
    return 0;
}
