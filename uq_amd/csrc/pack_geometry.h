// pack_geometry.h -- the tile geometry of pack_tile_kernel (pack.hip), worked out from an LDS budget in ONE place: reads per tile (R), reads per
// piece of a tile that does not fit the stage (Rs), lanes per read in phase B (P), the size of the staging region, the copies of the count table and
// the workgroups a CU holds.  Plain C++, no HIP types: pack_impl launches with it, uq_pack_tile_geometry reports it, and it compiles alone (the
// sweep of tools/pack_geometry_check.cpp runs it under the sanitizers).
//
// Two forms of the kernels exist (compile-time constants of the instances: DESIGN 10 and 22 record what run-time values cost there):
//   the standard tile   a 16 KiB stage with the statistics (20 KiB without): four (five) 16-byte vectors a lane in flight, at most 63 reads a tile --
//                       4 R + 1 line starts, one per lane --, which the rounding to a multiple of 16 makes 48;
//   the 64-read tile    a 22 KiB stage (six vectors a lane), 64 reads, four copies of the count table instead of eight: chosen where 64 records of the
//                       LONGEST kind fit the stage and the whole carve, static and dynamic, fits a quarter of the CU's LDS -- 2-bit bases in the fused forms built for
//                       four workgroups per CU, the 150 bp workloads.  Where it does not fit the geometry is the standard one, unchanged.
#pragma once
#include <cstdint>

namespace pkgeom {
constexpr uint32_t THREADS = 256;
constexpr uint32_t LDS_PER_CU = 160 * 1024;
constexpr uint32_t NV_PLAIN = 5, NV_STATS = 4, NV_TILE64 = 6;                  // 16-byte loads a lane holds in flight per tile
constexpr uint32_t STAGE_TILE64 = 22 * 1024;
constexpr uint32_t TILE64_READS = 64;                                           // (56 reads at this stage, 168 of the 192 lanes busy: 1.29 ms against 1.23 for the standard tile -- DESIGN 33)
constexpr uint32_t QNLDS_BYTES = 704, PARKED_BYTES = 64;                        // sizeof(QnLds), sizeof(PkParked) rounded to 16 (pack.hip asserts both)

// the staging region: what the lanes hold in flight (or the 22 KiB of the 64-read tile), and 32 bytes of slack for the windows
constexpr uint32_t stage_cap(bool stats, bool tile64) { return tile64 ? STAGE_TILE64 : (stats ? NV_STATS : NV_PLAIN) * THREADS * 16; }
constexpr uint32_t stage_bytes(bool stats, bool tile64) { return stage_cap(stats, tile64) + 32; }
constexpr uint32_t bins(int bd) { return bd == 3 ? 512u : 256u; }               // bin = base code << 6 | quality code (3-bit bases: nine bits)

struct Query {
    uint32_t bits_per_base, Cd, Cq;     // bytes per row
    uint32_t dna_max, variable;
    uint32_t max_record_bytes, avg_record_bytes;      // avg 0 = unknown
    bool stats, qn, ntrick, lists;      // the fused pack + statistics kernel; with the QNAME phase; an N-trick base; line starts from the census's lists
    bool one_copy;                      // (the PK_ONE_COPY tuning build)
};
struct Geometry {
    uint32_t tiled;                     // 0: the longest record does not fit a standard stage -- no tile kernel runs (the exact kernel, or no fused form)
    uint32_t tile64;
    uint32_t R, Rs, P, G;
    uint32_t stage_bytes, out_bytes, copies;
    uint32_t lds_dynamic, lds_static, lds_bytes;
    uint32_t wg_per_cu;                 // by the LDS (pack_impl lowers it where an instance's registers allow fewer)
};

inline uint32_t copies_of(const Query& q, bool four_wg, bool tile64) {
    if (q.one_copy) return q.bits_per_base == 3 ? 4 : 1;
    // (the forms built for four workgroups per CU have the LDS for eight copies of the 256 bins: DESIGN 11; the 64-read tile spends it on the stage)
    return q.bits_per_base == 2 && four_wg && !tile64 ? 8 : 4;
}
inline uint32_t round16(uint32_t x) { return (x + 15) & ~15u; }

inline void carve(const Query& q, bool four_wg, bool tile64, Geometry& g) {
    g.stage_bytes = stage_bytes(q.stats, tile64);
    g.out_bytes = round16(round16(g.R * q.Cd) + g.R * q.Cq);
    g.copies = q.stats ? copies_of(q, four_wg, tile64) : 0;
    // dynamic: [16 B guard][stage][luts 3 x 512 B][QnLds (statistics)][line offsets u32 x (4R+4)][out_d | out_q]; static: the count table and what is parked beside it
    g.lds_dynamic = 16 + g.stage_bytes + g.out_bytes + (4 * g.R + 4) * 4 + 3 * 512 + (q.stats ? QNLDS_BYTES : 0);
    g.lds_static = q.stats ? (bins((int)q.bits_per_base) * g.copies + 128) * 4 + (four_wg ? PARKED_BYTES : 0) : 4;
    g.lds_bytes = g.lds_dynamic + g.lds_static;
}

inline Geometry tile_geometry(const Query& q) {
    Geometry g{};
    const uint32_t rec = q.max_record_bytes, avg = q.avg_record_bytes;
    const uint32_t cap = stage_cap(q.stats, false);
    if (rec < 4 || rec + 64 > cap) return g;        // (records beyond the standard stage take the exact thread-per-read kernel)
    g.tiled = 1;
    g.G = (q.dna_max + (q.variable ? 1u : 0u) + 7) / 8;
    const bool four_wg = q.stats && (q.ntrick || q.qn);
    const uint32_t pack_lanes = q.qn ? THREADS - 64 : THREADS;         // (QNAME phase: the last wave parses lines instead)
    auto lanes_per_read = [&](uint32_t R) { uint32_t P = pack_lanes / R; if (P > g.G) P = g.G; return P < 1 ? 1u : P; };
    // the 64-read tile: 64 records of the longest kind, skew and slack in the stage; the carve within a quarter of the CU's LDS.  (Not the variable-length dealing
    // of the queued forms: its rows are sized for the longest read and do not fit.)
    if (four_wg && q.bits_per_base == 2 && !q.one_copy && !(q.lists && q.variable) && TILE64_READS * rec + 47 <= stage_bytes(true, true)) {
        Geometry b = g;
        b.tile64 = 1; b.R = b.Rs = TILE64_READS;
        carve(q, four_wg, true, b);
        if (b.lds_bytes <= LDS_PER_CU / 4) {
            b.P = lanes_per_read(b.R);
            b.wg_per_cu = 4;
            return b;
        }
    }
    // The standard tile.  Rs (from the LONGEST record) always fits the stage; R comes from the AVERAGE record (+15 %) when the caller knows it --
    // variable-length files fill the stage instead of leaving room for 48 longest reads -- and a tile whose records add up to more than the stage
    // is packed in pieces of Rs reads.
    const uint32_t most = (THREADS - 1) / 4;         // 4R + 1 line offsets, one per lane
    uint32_t Rs = (cap - 64) / rec;
    if (Rs > most) Rs = most;
    if (Rs == 0) Rs = 1;
    uint32_t R = Rs;
    if (avg >= 4 && avg < rec) {
        R = (cap - 64) / (avg + avg * 15 / 100 + 1);
        if (R > most) R = most;
        if (R < Rs) R = Rs;
    }
    // ... but the rows of a tile are sized for the LONGEST read: a file of short reads with a few long ones among them must not ask for
    // R rows of the long kind in LDS (a request beyond the CU's 160 KiB ended the call with an error instead of a slower tile)
    {
        const uint32_t out_cap = cap * 3 / 4, rowb = q.Cd + q.Cq, fit = rowb ? out_cap / rowb : R;
        if (R > fit) R = fit > Rs ? fit : Rs;
    }
    // R a multiple of 16 keeps every tile's output offset 16-byte aligned (uint4 stores); when that would waste
    // more than ~15 % of the tile, settle for a multiple of 8 or 4 (8- / 4-byte stores)
    if (R >= 4) {
        const uint32_t r16 = R & ~15u, r8 = R & ~7u, r4 = R & ~3u;
        if (r16 * 100 >= R * 85) R = r16; else if (r8 * 100 >= R * 85) R = r8; else R = r4;
    }
    if (R == 0) R = 1;
    if (Rs > R) Rs = R;
    g.R = R; g.Rs = Rs;
    carve(q, four_wg, false, g);
    g.P = lanes_per_read(R);
    uint32_t per_cu = g.lds_bytes <= LDS_PER_CU ? LDS_PER_CU / g.lds_bytes : 0;      // 0: the tile does not fit a CU at all (pack_impl refuses the call)
    if (per_cu > 6) per_cu = 6;
    g.wg_per_cu = per_cu;
    return g;
}
}  // namespace pkgeom
