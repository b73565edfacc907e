// plan_probe.cpp -- the planner (sprintz_amd/csrc/plan.h) on a host compiler, for tests/planner.py and through it every test that asks
// the planner: that this file builds with g++ is itself the check that plan.h and geom.h contain no HIP.  Reads one query per line from stdin,
//     decode|encode|dense|gather  key=value ...      (Shape fields and Knobs fields by name; what is not named keeps its default)
// and prints the plan -- the family by sprintz_mi355x_dispatch_name's table and every field -- or the error.  `sweep` runs the
// property sweep of tests/test_plan_cpu.py's docstring inside the probe and prints one line per violation, then the number of shapes;
// `modes` prints every kQuery* constant of geom.h as name=value.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

#include "../sprintz_amd/csrc/plan.h"

using namespace sprintz;

static std::string show(const Plan& p)
{
    char b[1024];
    if (p.err) { snprintf(b, sizeof b, "error=%d what=%s", p.err, p.what); return b; }
    snprintf(b, sizeof b, "family=%s grid=%llu lds=%llu dp=%d cpl=%d exact=%d ds=%d log2DP=%d lds_group_stride=%u vec_store=%d cap=%u chunks_per_group=%u "
             "lat_bound=%u norle=%d raw=%d quirk=%d lowdim=%d fire=%d fused=%d plain_memory=%d counters=%d table_off=%u wg_chunks=%u row=%u/%u/%u "
             "blkd=%u/%u/%u/%u blke=%u/%u/%u/%u",
             kFamilyNames[p.family], (unsigned long long)p.grid, (unsigned long long)p.lds, p.dp, p.cpl, (int)p.exact, p.ds, p.log2DP, p.lds_group_stride,
             p.vec_store, p.cap, p.chunks_per_group, p.lat_bound, p.norle, p.raw, p.quirk, (int)p.lowdim, (int)p.fire, (int)p.fused, (int)p.plain_memory,
             (int)p.counters, p.table_off, p.wg_chunks, p.row.U, p.row.G, p.row.ok, p.blkd.T, p.blkd.CPW, p.blkd.total, p.blkd.ok, p.blke.T, p.blke.CPW,
             p.blke.total, p.blke.ok);
    return b;
}

static bool set(Shape& s, Knobs& k, const std::string& key, unsigned long long v)
{
#define F(obj, name) if (key == #name) { obj.name = (decltype(obj.name))v; return true; }
    F(s, codec) F(s, esz) F(s, D) F(s, nchunks) F(s, chunk_len) F(s, total_len) F(s, noheader) F(s, q) F(s, general) F(s, col_stride) F(s, write_size)
    F(s, dense) F(s, host_call) F(s, src_lo) F(s, slots_lo) F(s, out_lo) F(s, comp_lo) F(s, slot_stride) F(s, nranges) F(s, rows) F(s, capacity) F(s, table_entries) F(s, table_row_max) F(s, out_esz)
    F(k, no_fast) F(k, lat_chunks) F(k, blk_chunks) F(k, blk_kernels) F(k, enc_pair) F(k, split_lanes) F(k, chunks_per_group) F(k, dense_mode) F(k, ref_quirk)
#undef F
    return false;
}

static unsigned long long g_bad = 0;
static void bad(const char* what, const Shape& s, const std::string& got)
{
    g_bad++;
    printf("violation: %s: codec=%d esz=%d D=%d chunk_len=%u nchunks=%llu -> %s\n", what, s.codec, s.esz, s.D, s.chunk_len, (unsigned long long)s.nchunks, got.c_str());
}

// one plan of the sweep: exactly one of plan and error, the same when asked twice, LDS and grid within the machine's limits
template <typename PlanFn> static Plan checked(PlanFn plan, const Shape& s, const Knobs& k)
{
    const Plan p = plan(s, k);
    const std::string a = show(p);
    if ((p.family >= 0) == (p.err != 0)) bad("both or neither of plan and error", s, a);
    if (a != show(plan(s, k))) bad("another answer the second time", s, a);
    if (!p.err && (p.lds > 160u * 1024u || p.grid < 1 || p.grid > 0x7fffffffull)) bad("LDS above 160 KB or grid outside 1 .. 2^31 - 1", s, a);
    return p;
}

static void sweep()
{
    unsigned long long shapes = 0;
    const uint64_t counts[] = {1, 64, 65, 2048, 2049, 131072};
    const Knobs def, nofast = [] { Knobs k; k.no_fast = 1; return k; }();
    for (int esz = 1; esz <= 2; esz++)
        for (int i = 1; i <= 516; i++) {
            const int D = i <= 512 ? i : i == 513 ? 513 : i == 514 ? 2047 : i == 515 ? 2048 : 65535;
            const uint32_t lens[] = {15u * D, 16u * D, 128u * D, (5120u + D - 1) / D * D, (10240u + D - 1) / D * D};
            for (uint32_t chunk_len : lens)
                for (uint64_t nchunks : counts)
                    for (int codec = SPRINTZ_CODEC_DELTA; codec <= SPRINTZ_CODEC_XFF; codec++) {
                        Shape s;
                        s.codec = codec; s.esz = esz; s.D = D; s.chunk_len = chunk_len; s.nchunks = nchunks; s.total_len = nchunks * chunk_len;
                        s.slot_stride = compress_bound(esz, chunk_len, (uint16_t)D);
                        shapes++;
                        const Plan d = checked(plan_decode, s, def), e = checked(plan_encode, s, def);
                        if (d.family == SPRINTZ_KF_DEC_FAST && !(d.dp * d.cpl >= D && 2 * D > d.dp * d.cpl)) bad("dec_fast: dp x cpl outside [D, 2 D)", s, show(d));
                        if (D <= 512) {
                            const Plan dn = checked(plan_decode, s, nofast), en = checked(plan_encode, s, nofast);
                            if (dn.family != SPRINTZ_KF_DEC_GENERIC) bad("no_fast: not dec_generic", s, show(dn));
                            if (en.family != SPRINTZ_KF_ENC_GENERIC) bad("no_fast: not enc_generic", s, show(en));
                        }
                        // the ticket path's agreement: with the host-call flag exactly the shapes that are dec_lat / enc_lat without it, one chunk
                        Shape one = s, host = s;
                        one.nchunks = host.nchunks = 1; one.total_len = host.total_len = chunk_len;
                        host.host_call = true;
                        if ((plan_decode(host, def).family == SPRINTZ_KF_DEC_LAT) != (plan_decode(one, def).family == SPRINTZ_KF_DEC_LAT)) bad("host call: dec_lat disagrees", s, show(plan_decode(host, def)));
                        if ((plan_encode(host, def).family == SPRINTZ_KF_ENC_LAT) != (plan_encode(one, def).family == SPRINTZ_KF_ENC_LAT)) bad("host call: enc_lat disagrees", s, show(plan_encode(host, def)));
                        (void)e;
                    }
        }
    printf("sweep shapes=%llu violations=%llu\n", shapes, g_bad);
}

// every kQuery* of geom.h on one line, for tests/planner.py's QUERY
static void modes()
{
#define M(name) printf(#name "=%d ", kQuery##name);
    M(Off) M(Materialize) M(ReduceOnly) M(Window) M(Gather) M(Filter) M(Select) M(Aggregate) M(Histogram) M(Moments) M(GroupBy) M(Extrema) M(Linear)
    M(Segment) M(Float)
#undef M
    printf("\n");
}

int main()
{
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string op, tok;
        if (!(in >> op)) continue;
        if (op == "sweep") { sweep(); continue; }
        if (op == "modes") { modes(); continue; }
        Shape s;
        Knobs k;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos || !set(s, k, tok.substr(0, eq), strtoull(tok.c_str() + eq + 1, nullptr, 0))) { printf("bad token %s\n", tok.c_str()); return 2; }
        }
        if (op == "decode") puts(show(plan_decode(s, k)).c_str());
        else if (op == "encode") puts(show(plan_encode(s, k)).c_str());
        else if (op == "gather") puts(show(plan_gather(s, k)).c_str());
        else if (op == "dense") {
            Plan enc;
            const Plan d = plan_dense(s, k, &enc);
            if (d.err) puts(show(d).c_str());
            else printf("family=%s enc=%s\n", kFamilyNames[d.family], enc.family >= 0 ? kFamilyNames[enc.family] : "none");
        } else { printf("bad op %s\n", op.c_str()); return 2; }
    }
    return 0;
}
