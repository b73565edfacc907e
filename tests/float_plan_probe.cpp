// float_plan_probe.cpp -- plan_decode (sprintz_amd/csrc/plan.h) for the float-rows mode on a host compiler, for
// tests/test_float_cpu.py and tests/test_gpu_float_rows.py.  One query per line on stdin,
//     esz=.. D=.. chunk_len=.. nchunks=.. codec=.. out_esz=.. out_lo=.. no_fast=.. general=.. chunks_per_group=.. blk_chunks=.. lat_chunks=..
// (out_esz: 4 for float32, 2 for float16 / bfloat16; out_lo: the low four bits of the output's address) and one answer per line: the
// family's name, the launch's dynamic LDS bytes, its grid, lanes a chunk, columns a lane, chunks a lane group and vec_store -- or the error.
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>

#include "../sprintz_amd/csrc/plan.h"

using namespace sprintz;

int main()
{
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string tok;
        Shape s;
        Knobs k;
        s.q = kQueryFloat;
        s.out_esz = 4;
        bool any = false;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { printf("bad token %s\n", tok.c_str()); return 2; }
            const std::string key = tok.substr(0, eq);
            const unsigned long long v = strtoull(tok.c_str() + eq + 1, nullptr, 0);
            any = true;
            if (key == "esz") s.esz = (int)v;
            else if (key == "D") s.D = (int)v;
            else if (key == "codec") s.codec = (int)v;
            else if (key == "chunk_len") s.chunk_len = (uint32_t)v;
            else if (key == "nchunks") s.nchunks = v;
            else if (key == "general") s.general = (int)v;
            else if (key == "out_esz") s.out_esz = (int)v;
            else if (key == "out_lo") s.out_lo = (unsigned)v & 15u;
            else if (key == "no_fast") k.no_fast = (int)v;
            else if (key == "chunks_per_group") k.chunks_per_group = (int)v;
            else if (key == "blk_chunks") k.blk_chunks = (int)v;
            else if (key == "lat_chunks") k.lat_chunks = (int)v;
            else { printf("bad key %s\n", key.c_str()); return 2; }
        }
        if (!any) continue;
        const Plan p = plan_decode(s, k);
        if (p.err) printf("error=%d\n", p.err);
        else
            printf("%s lds=%llu grid=%llu log2dp=%d cpl=%d dp=%d exact=%d cpg=%u vec=%d\n", kFamilyNames[p.family], (unsigned long long)p.lds,
                   (unsigned long long)p.grid, p.log2DP, p.cpl, p.dp, (int)p.exact, p.chunks_per_group, p.vec_store);
    }
    return 0;
}
