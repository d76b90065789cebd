// pack_geometry_check.cpp -- the pack kernels' tile geometry (uq_amd/csrc/pack_geometry.h) swept over record lengths, row sizes, average records and
// kernel forms on the host, under the sanitizers:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I uq_amd/csrc tools/pack_geometry_check.cpp -o pack_geometry_check
//     ./pack_geometry_check
// Every point that has a tile must keep what the kernel relies on: the carve within the CU's LDS divided by the workgroups it reports, Rs records of
// the longest kind (the 64-read tile: R of them) with skew and slack inside the stage, 1 <= P <= G, P lanes for each of R reads among the lanes that
// pack, Rs <= R <= 64, a line start per lane.  Prints the points visited; exit status 1 and the first failing point otherwise.
// (tests/test_pack_geometry_cpu.py builds and runs it, and asks the library's query the same questions.)
#include <cstdio>
#include <cstdlib>

#include "pack_geometry.h"

static unsigned long long points = 0, tiled = 0, tile64 = 0;

static void fail(const pkgeom::Query& q, const pkgeom::Geometry& g, const char* what) {
    std::printf("FAILED: %s\n  query: bd %u Cd %u Cq %u dna_max %u variable %u rec %u avg %u stats %d qn %d ntrick %d lists %d\n"
                "  geometry: tiled %u tile64 %u R %u Rs %u P %u G %u stage %u out %u copies %u lds %u (+%u static) wg %u\n",
                what, q.bits_per_base, q.Cd, q.Cq, q.dna_max, q.variable, q.max_record_bytes, q.avg_record_bytes, (int)q.stats, (int)q.qn, (int)q.ntrick,
                (int)q.lists, g.tiled, g.tile64, g.R, g.Rs, g.P, g.G, g.stage_bytes, g.out_bytes, g.copies, g.lds_bytes, g.lds_static, g.wg_per_cu);
    std::exit(1);
}
#define CHECK(c) do { if (!(c)) fail(q, g, #c); } while (0)

static void point(const pkgeom::Query& q) {
    const pkgeom::Geometry g = pkgeom::tile_geometry(q);
    ++points;
    const uint32_t rec = q.max_record_bytes;
    CHECK((g.tiled != 0) == (rec >= 4 && rec + 64 <= pkgeom::stage_cap(q.stats, false)));
    if (!g.tiled) { CHECK(g.R == 0 && g.lds_bytes == 0); return; }
    ++tiled;
    CHECK(g.wg_per_cu >= 1 && g.wg_per_cu <= 6);
    CHECK((unsigned long long)g.lds_bytes * g.wg_per_cu <= pkgeom::LDS_PER_CU);
    CHECK(g.lds_bytes == g.lds_dynamic + g.lds_static);
    CHECK(g.Rs >= 1 && g.Rs <= g.R && g.R <= 64);
    CHECK((unsigned long long)g.Rs * rec + 47 <= g.stage_bytes);
    // (a tile sized from the AVERAGE record may exceed the stage: that is what the pieces of Rs reads are for; without an average it may not)
    if (g.tile64 || q.avg_record_bytes < 4 || q.avg_record_bytes >= rec) CHECK((unsigned long long)g.R * rec + 47 <= g.stage_bytes);
    CHECK(g.G == (q.dna_max + q.variable + 7) / 8);
    CHECK(g.P >= 1 && g.P <= g.G);
    const uint32_t lanes = q.qn ? pkgeom::THREADS - 64 : pkgeom::THREADS;
    CHECK(g.P * g.R <= lanes || g.P == 1);
    CHECK(g.out_bytes >= g.R * (q.Cd + q.Cq) && g.out_bytes % 16 == 0 && g.stage_bytes % 16 == 0);
    if (g.tile64) {
        ++tile64;
        CHECK(g.R == pkgeom::TILE64_READS && g.Rs == g.R && g.wg_per_cu == 4 && g.copies == 4 && g.stage_bytes == pkgeom::STAGE_TILE64 + 32);
        CHECK(q.stats && (q.qn || q.ntrick) && q.bits_per_base == 2 && !(q.lists && q.variable));
        CHECK(4 * g.R <= pkgeom::THREADS);                    // line starts 1 .. 4R, one per lane (start 0 is the tile's own)
        CHECK(g.lds_bytes <= pkgeom::LDS_PER_CU / 4);
    } else {
        CHECK(4 * g.R + 1 <= pkgeom::THREADS);                // line starts 0 .. 4R, one per lane
        CHECK(g.stage_bytes == pkgeom::stage_bytes(q.stats, false));
    }
}

int main() {
    static const uint32_t bq_of[] = {1, 2, 3, 4, 5, 6, 8};
    for (uint32_t rec = 8; rec <= 20000; rec += rec < 420 ? 1 : rec < 2000 ? 13 : 197) {
        // reads a record of this size can hold: one symbol, a few, and the longest (two lines of L + 1 bytes, a QNAME line and "+\n" of two bytes each at least)
        const uint32_t Lmax = (rec - 6) / 2;
        const uint32_t Ls[] = {1, 7, 8, 36, 150, Lmax / 2, Lmax};
        for (uint32_t L : Ls) {
            if (L < 1 || L > Lmax) continue;
            for (uint32_t variable = 0; variable < 2; ++variable)
                for (uint32_t bd = 2; bd <= 3; ++bd)
                    for (uint32_t bq : bq_of) {
                        pkgeom::Query q{};
                        q.bits_per_base = bd; q.dna_max = L; q.variable = variable;
                        q.Cd = (bd * (L + variable) + 7) / 8; q.Cq = (bq * (L + variable) + 7) / 8;
                        if (q.Cd + q.Cq > 400) continue;          // rows up to 400 bytes
                        q.max_record_bytes = rec;
                        const uint32_t avgs[] = {0, 4, rec / 3, rec / 2, rec - rec / 8, rec - 1, rec};
                        for (uint32_t avg : avgs) {
                            q.avg_record_bytes = avg;
                            for (int form = 0; form < 5; ++form) {        // plain; statistics; + QNAME; + lists; + QNAME + lists
                                q.stats = form >= 1; q.qn = form == 2 || form == 4; q.lists = form >= 3;
                                for (int nt = 0; nt < 2; ++nt) { q.ntrick = nt != 0; point(q); }
                            }
                        }
                    }
        }
    }
    std::printf("pack geometry: %llu points, %llu tiled, %llu with the 64-read tile: ok\n", points, tiled, tile64);
    return tile64 && tiled > tile64 ? 0 : 1;
}
