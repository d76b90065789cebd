// qc.hip -- the per-cycle quality control tables `uqqc1` (the definition stands in include/uqhip.h): base class and Phred
// counts per position in the read, read-length, mean-quality and GC histograms, five scalars.  An extension: the reference has no such pass.
//
// The kernel reads the stream once and writes nothing but d_qc.  Workgroups are persistent (one per CU) and walk over groups of G
// consecutive records, G sized on the device from the shard's average record length so that a typical group is one LDS tile.  A group's byte
// span is staged tile by tile as in fingerprint.hip (QC_TILE bytes, cut at 16-byte-aligned addresses, one 16-byte coalesced load per lane, the
// next tile in flight in registers while this one is counted); a byte belongs to the tile that holds it.
//
// The bins are indexed by the position in the read, so the 64 lanes of a wave walk 64 CONSECUTIVE positions of ONE line: position p of the
// SEQ line and position p of the QUAL line in the same step.  The workgroup's private table is column-major, tab[column][cycle] with
// QC_LDS_CYCLES a multiple of 32: the bank of a cell is its cycle mod 32 whatever the column, and the two 32-lane halves that a ds_add_u32 is
// served in never meet -- no wave instruction collides on a bank, whatever the bases and qualities are.  A group of G >= 16 records deals whole
// records to the 16 waves; smaller groups (long reads) deal the 64-position chunks of a record to 16 / G waves each, so a 70 kbp read is
// spread over all lanes of the workgroup -- never a per-thread loop over HBM along a line.  A byte becomes its column and what it adds to the
// read's sums (G/C count, Phred sum) through two 256-entry tables in LDS; the sums are reduced over the wave in registers (DPP).  The usual
// group lies in its first tile and takes a form of the record loop with 32-bit offsets; groups of several tiles take the general one.
//
// LDS per workgroup (160 KiB per CU): the table (6 + 94) x QC_LDS_CYCLES u32 = 128 000 B, the tail row 400 B, the staging tile 16 384 B, the
// group's line starts 6 168 B (twice: 64-bit, and 32-bit from the group's first byte), per-read sums 1 536 B, the three small histograms
// 2 064 B, scalars 40 B, two byte tables 4 096 B: 158 688 B.  That is ONE workgroup of 1024 lanes per CU: 16 waves per CU, 4 per SIMD
// (which its 89 VGPRs admit as well).
// Exact cycles [QC_LDS_CYCLES, C) -- the long-read path, sized for correctness -- go straight to d_qc by global atomics; the tail row (cycles
// >= C) is always counted in LDS.  The table is flushed (non-zero cells, u64 global atomic adds) at the end and after every QC_FLUSH_TILES
// tiles: a tile adds at most QC_TILE to any one cell and a group at most QC_GMAX to a histogram cell, so no u32 counter reaches
// 2^17 * 16 384 + 128 < 2^32 between two flushes.
// Algorithmic HBM bytes: the record bytes once + 32 B of line offsets per record.
#include "common.h"

namespace {
constexpr int QC_THREADS = 1024;
constexpr uint32_t QC_WAVES = QC_THREADS / 64;
constexpr uint32_t QC_TILE = 16384;                  // bytes of the stream per staged tile: one 16-byte vector per lane
constexpr uint32_t QC_NV = QC_TILE / 16;
static_assert((QC_TILE & (QC_TILE - 1u)) == 0, "an offset into the staging tile is masked with QC_TILE - 1");
constexpr uint32_t QC_LDS_CYCLES = 320;              // exact cycles counted in LDS (tests/test_gpu_qc.py builds its inputs from this)
constexpr uint32_t QC_GMAX = 128;                    // records per group, upper bound: its 4 G + 1 line starts are one per lane
constexpr uint32_t QC_FLUSH_TILES = 1u << 17;
constexpr uint32_t QC_COLS = UQ_QC_NBASE + UQ_QC_NQUAL;

// cls(b) without a branch: 5 - cls of the letters 'a' .. 'u' in three bits each (a: 5, c: 4, g: 3, t: 2, n: 1, the others 0); every other byte
// takes slot 21, whose one bit in the word is 0
__host__ __device__ __forceinline__ uint32_t qc_cls(uint32_t b) {
    constexpr uint64_t T = (5ull << 0) | (4ull << 3 * 2) | (3ull << 3 * 6) | (1ull << 3 * 13) | (2ull << 3 * 19);
    const uint32_t i = (b | 0x20u) - 'a';
    return 5u - ((uint32_t)(T >> (3u * (i < 21u ? i : 21u))) & 7u);
}
__host__ __device__ __forceinline__ uint32_t qc_phred(uint32_t b) { return b < 33u ? 0u : (b > 126u ? 93u : b - 33u); }

// offsets (in u64 words) of the object's parts
__host__ __device__ __forceinline__ uint64_t qc_off_base(uint32_t) { return 8; }
__host__ __device__ __forceinline__ uint64_t qc_off_qual(uint32_t C) { return 8 + (uint64_t)UQ_QC_NBASE * (C + 1); }
__host__ __device__ __forceinline__ uint64_t qc_off_len(uint32_t C) { return 8 + (uint64_t)QC_COLS * (C + 1); }
__host__ __device__ __forceinline__ uint64_t qc_off_mq(uint32_t C) { return qc_off_len(C) + (C + 1); }
__host__ __device__ __forceinline__ uint64_t qc_off_gc(uint32_t C) { return qc_off_mq(C) + UQ_QC_NQUAL; }

// a value every lane of the wave holds, moved to SGPRs: what is computed from it costs no vector instruction and branches without a mask
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
}
__device__ __forceinline__ uint32_t uni32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }
// the sum over the wave's 64 lanes, in every lane: four DPP steps inside the rows of 16 lanes (no LDS instruction, unlike a shuffle: the LDS
// pipeline is what this kernel is short of), then the four row sums read lane by lane.  Every lane of the wave must be active.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);     // quad_perm [1, 0, 3, 2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);     // quad_perm [2, 3, 0, 1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0xF, false);    // row_ror:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);    // row_ror:8
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

__global__ __launch_bounds__(QC_THREADS) void qc_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ ls, uint64_t first, uint64_t n,
                                                         uint32_t C, unsigned long long* __restrict__ qc) {
    __shared__ uint32_t tab[QC_COLS * QC_LDS_CYCLES];           // [column][cycle]: columns 0..5 the base classes, 6..99 the Phred values
    __shared__ uint32_t tail[QC_COLS];                          // the row of the positions >= C
    __shared__ __align__(16) uint8_t stage[QC_NV * 16];
    __shared__ uint64_t meta[4 * QC_GMAX + 1];                  // line starts of the group's records (stream offsets)
    __shared__ __align__(16) uint32_t m32[4 * QC_GMAX + 4];     // the same as offsets from the group's t0, entry k at k + 3: a record's last four are one aligned vector
    __shared__ unsigned long long rsq[QC_GMAX];                 // per record of the group: the sum of its Phred values ...
    __shared__ uint32_t rgc[QC_GMAX];                           // ... and the number of its G and C
    __shared__ uint32_t lenh[QC_LDS_CYCLES + 1], mqh[UQ_QC_NQUAL], gch[101];    // lenh[QC_LDS_CYCLES]: the reads of C bases and more
    __shared__ unsigned long long sacc[5];                      // reads, bases, qual_chars, qual_out_of_range, len_mismatch
    // byte -> {the byte offset of its column in tab, what it adds to the lane's sums}: one LDS read instead of a dozen vector instructions a
    // position (the vector unit, four cycles an instruction, is what the counting loop is short of)
    __shared__ uint2 lut_s[256], lut_u[256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    // the launch geometry is decided here (no device -> host round trip before the launch), the same in every workgroup
    const uint64_t lo = ls[4 * first], hi = ls[4 * (first + n)];                 // the shard's bytes: nothing outside [lo, hi) is loaded
    const uint64_t avg = (hi - lo) / n + 1;
    const uint64_t G64 = (QC_TILE - 64) / (avg + avg / 8 + 1);
    const uint32_t G = (uint32_t)(G64 > QC_GMAX ? QC_GMAX : (G64 < 1 ? 1 : G64));
    const uint32_t WPR = G >= QC_WAVES ? 1u : QC_WAVES / G;                      // waves per record
    const uint32_t rr0 = wave / WPR, rstep = QC_WAVES / WPR, sub = wave - rr0 * WPR;
    const uint32_t Cl = C < QC_LDS_CYCLES ? C : QC_LDS_CYCLES;                   // exact cycles [0, Cl) are counted in LDS
    const uint64_t ngroups = (n + G - 1) / G, S = gridDim.x;
    const uint64_t abase = (uint64_t)(uintptr_t)buf;
    unsigned long long* const qbase = qc + qc_off_base(C);
    unsigned long long* const qqual = qc + qc_off_qual(C);

    uint64_t g = blockIdx.x;
    if (g >= ngroups) return;

    // Tiles as in fingerprint.hip: a group's tile c covers the stream offsets [cb, cb + QC_TILE), cb = t0 + c * QC_TILE, t0 <= the group's
    // first byte at a 16-byte-aligned ADDRESS (negative when the buffer itself is misaligned).
    struct Regs { uint4 v; uint64_t m; };
    static_assert(4 * QC_GMAX + 1 <= QC_THREADS, "one line start per lane");
    static_assert(QC_NV == QC_THREADS, "one vector per lane");
    static_assert(QC_LDS_CYCLES % 32 == 0 && QC_LDS_CYCLES >= 301, "the bank of a cell is its cycle mod 32; the benchmark's short reads fit");
    auto group_t0 = [&](uint64_t gg) { return (int64_t)(((abase + ls[4 * (first + gg * G)]) & ~uint64_t(15)) - abase); };
    auto issue_tile = [&](Regs& x, int64_t cb, int64_t end) {                    // end: nothing at or beyond it is wanted (<= hi)
        const int64_t o = cb + 16 * (int64_t)tid;                                // a vector is loaded iff it holds a byte of the shard: it shares that byte's page
        x.v = (o + 16 > (int64_t)lo && o < end) ? *(const uint4*)(buf + o) : make_uint4(0, 0, 0, 0);
    };
    auto issue_meta = [&](Regs& x, uint64_t gg) {
        const uint64_t r0 = gg * G;
        const uint32_t Rt = (uint32_t)((n - r0) < G ? (n - r0) : G);
        const uint64_t* lsp = ls + 4 * (first + r0);
        x.m = tid <= 4 * Rt ? lsp[tid] : 0;
    };
    // non-zero cells -> d_qc, and the table is zero again (the caller puts barriers around it)
    auto flush = [&](uint32_t& oor) {
        for (uint32_t i = tid; i < QC_COLS * QC_LDS_CYCLES; i += QC_THREADS) {
            const uint32_t v = tab[i];
            if (v) {
                const uint32_t col = i / QC_LDS_CYCLES, row = i - col * QC_LDS_CYCLES;
                tab[i] = 0;
                if (col < UQ_QC_NBASE) atomicAdd(qbase + (uint64_t)row * UQ_QC_NBASE + col, (unsigned long long)v);
                else atomicAdd(qqual + (uint64_t)row * UQ_QC_NQUAL + (col - UQ_QC_NBASE), (unsigned long long)v);
            }
        }
        if (tid < QC_COLS) {
            const uint32_t v = tail[tid];
            tail[tid] = 0;
            if (v) {
                if (tid < UQ_QC_NBASE) atomicAdd(qbase + (uint64_t)C * UQ_QC_NBASE + tid, (unsigned long long)v);
                else atomicAdd(qqual + (uint64_t)C * UQ_QC_NQUAL + (tid - UQ_QC_NBASE), (unsigned long long)v);
            }
        }
        if (tid <= QC_LDS_CYCLES) {
            const uint32_t v = lenh[tid];
            lenh[tid] = 0;
            if (v) atomicAdd(qc + qc_off_len(C) + (tid < QC_LDS_CYCLES ? tid : C), (unsigned long long)v);
        }
        if (tid < UQ_QC_NQUAL) { const uint32_t v = mqh[tid]; mqh[tid] = 0; if (v) atomicAdd(qc + qc_off_mq(C) + tid, (unsigned long long)v); }
        if (tid < 101) { const uint32_t v = gch[tid]; gch[tid] = 0; if (v) atomicAdd(qc + qc_off_gc(C) + tid, (unsigned long long)v); }
        if (oor) { atomicAdd(&sacc[3], (unsigned long long)oor); oor = 0; }
    };

    for (uint32_t i = tid; i < QC_COLS * QC_LDS_CYCLES; i += QC_THREADS) tab[i] = 0;
    if (tid < QC_COLS) tail[tid] = 0;
    if (tid <= QC_LDS_CYCLES) lenh[tid] = 0;
    if (tid < UQ_QC_NQUAL) mqh[tid] = 0;
    if (tid < 101) gch[tid] = 0;
    if (tid < 5) sacc[tid] = 0;
    if (tid < 256) {
        const uint32_t c = qc_cls(tid), q = qc_phred(tid);
        lut_s[tid] = make_uint2(c * QC_LDS_CYCLES * 4u, ((c == 1u || c == 2u) ? 1u : 0u) | (c << 16));
        lut_u[tid] = make_uint2((UQ_QC_NBASE + q) * QC_LDS_CYCLES * 4u, q | ((tid < 33u || tid > 126u) ? 1u << 16 : 0u));
    }

    Regs cur;
    int64_t t0 = group_t0(g), t0n = g + S < ngroups ? group_t0(g + S) : 0;
    issue_meta(cur, g);
    issue_tile(cur, t0, (int64_t)hi);
    uint32_t oor = 0, ntiles = 0;
    unsigned long long nbases = 0, nquals = 0, nmis = 0, nreads = 0;
    for (; g < ngroups; g += S) {
        const uint64_t r0 = g * G;
        const uint32_t Rt = (uint32_t)((n - r0) < G ? (n - r0) : G);
        const bool more = g + S < ngroups;
        const int64_t t0nn = g + 2 * S < ngroups ? group_t0(g + 2 * S) : 0;      // (a scalar load, asked for two groups ahead: nobody waits for it here)
        if (tid <= 4 * Rt) { meta[tid] = cur.m; m32[tid + 3] = (uint32_t)((int64_t)cur.m - t0); }     // (m32: mod 2^32; the offsets themselves where the group is one tile)
        if (tid < Rt) { rsq[tid] = 0; rgc[tid] = 0; }
        for (int64_t cb = t0;; cb += QC_TILE) {                                   // (a group has at least one tile)
            const int64_t ce = cb + QC_TILE;
            if (cb != t0) __syncthreads();                                        // the previous tile has been read
            ((uint4*)stage)[tid] = cur.v;
            __syncthreads();
            // the end of the group's span, out of LDS and kept wave-uniform (in SGPRs): a load from HBM here would stall every group's start
            const int64_t g1 = (int64_t)uni64(meta[4 * Rt]);
            const bool last = ce >= g1;
            if (!last) issue_tile(cur, ce, g1);
            else if (more) { issue_meta(cur, g + S); issue_tile(cur, t0n, (int64_t)hi); }
            // The usual group lies in its first tile: every offset from t0 fits 32 bits, every line is whole, and a record costs a fraction
            // of the instructions of the general form below.  (rr and everything derived from the line starts is wave-uniform, in SGPRs.)
            if (cb == t0 && last) for (uint32_t rr = rr0; rr < Rt; rr += rstep) {
                const uint4 m = *(const uint4*)&m32[4 * rr + 4];                  // the offsets of SEQ, '+', QUAL and the next record from t0
                const uint32_t so = uni32(m.x), sp = uni32(m.y), uo = uni32(m.z), e = uni32(m.w);
                const uint32_t Ls = sp - so - 1u, Lu = e - uo - 1u, Lmax = Ls > Lu ? Ls : Lu, Lmin = Ls < Lu ? Ls : Lu;
                uint32_t accs = 0, accu = 0;
                for (uint32_t d0 = sub * 64u; d0 < Lmax; d0 += 64u * WPR) {
                    const uint32_t p = d0 + lane;
                    const uint2 es = lut_s[stage[(so + p) & (QC_TILE - 1u)]], eu = lut_u[stage[(uo + p) & (QC_TILE - 1u)]];
                    if (d0 + 64u <= Cl) {                                         // 64 cycles of the LDS table
                        if (d0 + 64u <= Lmin) {                                   // ... in both lines: no lane is masked
                            atomicAdd((uint32_t*)((char*)tab + (es.x + 4u * p)), 1u);
                            atomicAdd((uint32_t*)((char*)tab + (eu.x + 4u * p)), 1u);
                            accs += es.y; accu += eu.y;
                        } else {
                            if (p < Ls) { atomicAdd((uint32_t*)((char*)tab + (es.x + 4u * p)), 1u); accs += es.y; }
                            if (p < Lu) { atomicAdd((uint32_t*)((char*)tab + (eu.x + 4u * p)), 1u); accu += eu.y; }
                        }
                    } else {
                        if (p < Ls) {
                            accs += es.y;
                            if (p < Cl) atomicAdd((uint32_t*)((char*)tab + (es.x + 4u * p)), 1u);
                            else if (p >= C) atomicAdd(&tail[es.y >> 16], 1u);
                            else atomicAdd(qbase + (uint64_t)p * UQ_QC_NBASE + (es.y >> 16), 1ull);
                        }
                        if (p < Lu) {
                            accu += eu.y;
                            if (p < Cl) atomicAdd((uint32_t*)((char*)tab + (eu.x + 4u * p)), 1u);
                            else if (p >= C) atomicAdd(&tail[UQ_QC_NBASE + (eu.y & 0xFFFFu)], 1u);
                            else atomicAdd(qqual + (uint64_t)p * UQ_QC_NQUAL + (eu.y & 0xFFFFu), 1ull);
                        }
                    }
                }
                oor += accu >> 16;
                uint32_t gc = accs & 0xFFFFu, sq = accu & 0xFFFFu;
                if (Lmax <= 2048u) {                                              // sum q <= 93 * 2048 < 2^20: one reduction for both
                    const uint32_t t = wave_sum_u32(sq | (gc << 20));
                    sq = t & 0xFFFFFu; gc = t >> 20;
                } else {
                    gc = wave_sum_u32(gc);
                    sq = wave_sum_u32(sq);
                }
                if (lane == 0) {
                    if (gc) atomicAdd(&rgc[rr], gc);
                    if (sq) atomicAdd(&rsq[rr], (unsigned long long)sq);
                }
            }
            else for (uint32_t rr = rr0; rr < Rt; rr += rstep) {
                const int64_t ss = (int64_t)uni64(meta[4 * rr + 1]), sp = (int64_t)uni64(meta[4 * rr + 2]), su = (int64_t)uni64(meta[4 * rr + 3]),
                              e = (int64_t)uni64(meta[4 * rr + 4]);
                if (ss >= ce || e <= cb) continue;                                // the record has no SEQ or QUAL byte in this tile
                const uint32_t Ls = (uint32_t)(sp - ss - 1), Lu = (uint32_t)(e - su - 1);
                // the positions of the two lines that lie in this tile: [slo, shi) of SEQ, [ulo, uhi) of QUAL (lo == hi: none)
                auto clip = [&](int64_t s, uint32_t L, uint32_t& a, uint32_t& b) {
                    const int64_t x = cb - s, y = ce - s;
                    a = x <= 0 ? 0u : (x < (int64_t)L ? (uint32_t)x : L);
                    b = y <= 0 ? 0u : (y < (int64_t)L ? (uint32_t)y : L);
                };
                uint32_t slo, shi, ulo, uhi;
                clip(ss, Ls, slo, shi);
                clip(su, Lu, ulo, uhi);
                const uint32_t so = (uint32_t)(ss - cb), uo = (uint32_t)(su - cb);       // mod 2^32: so + p lies in [0, QC_TILE) for every p in [slo, shi)
                // One pass over the union of the two ranges where they overlap (a record inside the tile: both are [0, L)), else one pass each.
                // A pass walks [a, b) (b - a <= QC_TILE) in steps of 64 consecutive positions, dealt round robin to the record's WPR waves.
                const bool both = (slo > ulo ? slo : ulo) < (shi < uhi ? shi : uhi);
                const uint32_t pa[2] = {both ? (slo < ulo ? slo : ulo) : slo, both ? 0u : ulo}, pb[2] = {both ? (shi > uhi ? shi : uhi) : shi, both ? 0u : uhi};
                // this lane's share, summed as the tables' second words come: accs = #G/C | sum cls << 16, accu = sum q | #out of range << 16
                // (at most QC_TILE / 64 = 256 positions per lane, record and tile: sum q <= 23 808, no field runs into the next)
                uint32_t accs = 0, accu = 0;
                for (int pass = 0; pass < 2; ++pass) {
                    const uint32_t a = pa[pass], len = pb[pass] - a;
                    for (uint32_t d0 = sub * 64u; d0 < len; d0 += 64u * WPR) {
                        const uint32_t d = d0 + lane, p = a + d;
                        const uint64_t p0 = (uint64_t)a + d0;
                        if (p0 >= (slo > ulo ? slo : ulo) && p0 + 64u <= (shi < uhi ? shi : uhi) && p0 + 64u <= Cl) {
                            // all 64 positions lie in both lines and in the LDS table: no lane is masked, no lane takes another way
                            const uint2 es = lut_s[stage[so + p]], eu = lut_u[stage[uo + p]];
                            atomicAdd((uint32_t*)((char*)tab + (es.x + 4u * p)), 1u);
                            atomicAdd((uint32_t*)((char*)tab + (eu.x + 4u * p)), 1u);
                            accs += es.y; accu += eu.y;
                            continue;
                        }
                        // (d < len keeps p from wrapping at the end of a line of almost 2^32 bytes)
                        const bool in_s = d < len && p >= slo && p < shi, in_u = d < len && p >= ulo && p < uhi;
                        const uint2 es = lut_s[stage[(so + p) & (QC_TILE - 1u)]], eu = lut_u[stage[(uo + p) & (QC_TILE - 1u)]];
                        if (in_s) {
                            const uint32_t c = es.y >> 16;
                            accs += es.y;
                            if (p < Cl) atomicAdd((uint32_t*)((char*)tab + (es.x + 4u * p)), 1u);
                            else if (p >= C) atomicAdd(&tail[c], 1u);
                            else atomicAdd(qbase + (uint64_t)p * UQ_QC_NBASE + c, 1ull);
                        }
                        if (in_u) {
                            const uint32_t q = eu.y & 0xFFFFu;
                            accu += eu.y;
                            if (p < Cl) atomicAdd((uint32_t*)((char*)tab + (eu.x + 4u * p)), 1u);
                            else if (p >= C) atomicAdd(&tail[UQ_QC_NBASE + q], 1u);
                            else atomicAdd(qqual + (uint64_t)p * UQ_QC_NQUAL + q, 1ull);
                        }
                    }
                }
                oor += accu >> 16;
                uint32_t gc = accs & 0xFFFFu, sq = accu & 0xFFFFu;
                gc = wave_sum_u32(gc);
                sq = wave_sum_u32(sq);
                if (lane == 0) {
                    if (gc) atomicAdd(&rgc[rr], gc);
                    if (sq) atomicAdd(&rsq[rr], (unsigned long long)sq);
                }
            }
            if (++ntiles == QC_FLUSH_TILES) {                                     // (uniform over the workgroup)
                __syncthreads();
                flush(oor);
                ntiles = 0;
            }
            if (last) break;
        }
        __syncthreads();
        if (tid < Rt) {                                                           // one lane per read bins its per-read quantities
            const uint32_t ss = m32[tid * 4 + 4], sp = m32[tid * 4 + 5], su = m32[tid * 4 + 6], e = m32[tid * 4 + 7];     // (differences of neighbours: exact mod 2^32 in every group)
            const uint32_t Ls = sp - ss - 1u, Lu = e - su - 1u;
            nbases += Ls; nquals += Lu; nmis += Ls != Lu; nreads += 1;            // (this lane's, to the end of the kernel)
            if (Ls < Cl) atomicAdd(&lenh[Ls], 1u);
            else if (Ls >= C) atomicAdd(&lenh[QC_LDS_CYCLES], 1u);
            else atomicAdd(qc + qc_off_len(C) + Ls, 1ull);
            // (both quotients from 32-bit divisions wherever the dividends fit them: a 64-bit one is some 200 instructions)
            if (Lu) atomicAdd(&mqh[Lu < (1u << 25) ? (uint32_t)rsq[tid] / Lu : (uint32_t)(rsq[tid] / Lu)], 1u);
            if (Ls) atomicAdd(&gch[Ls < (1u << 25) ? 100u * rgc[tid] / Ls : (uint32_t)(100ull * rgc[tid] / Ls)], 1u);
        }
        __syncthreads();                                                          // meta, the per-read sums and the staging buffer are free again
        t0 = t0n; t0n = t0nn;
    }
    flush(oor);
    if (nreads) { atomicAdd(&sacc[0], nreads); atomicAdd(&sacc[1], nbases); atomicAdd(&sacc[2], nquals); if (nmis) atomicAdd(&sacc[4], nmis); }
    __syncthreads();
    if (tid < 5 && sacc[tid]) atomicAdd(qc + tid, sacc[tid]);                     // one atomic per field per workgroup
}
}  // namespace

extern "C" uint64_t uq_qc_words(uint32_t ncycles) {
    if (ncycles < 1 || ncycles > UQ_QC_MAX_CYCLES) return 0;
    return qc_off_gc(ncycles) + 101;
}

extern "C" int uq_qc_init(uq_ctx* ctx, uint64_t* d_qc, uint32_t ncycles) {
    UQ_REQUIRE(ctx && d_qc, "uq_qc_init: null argument");
    UQ_REQUIRE(uq_qc_words(ncycles) != 0, "uq_qc_init: ncycles = %u is outside 1 .. %u", ncycles, (unsigned)UQ_QC_MAX_CYCLES);
    UQ_CHECK_HIP(hipMemsetAsync(d_qc, 0, uq_qc_words(ncycles) * 8, ctx->stream));
    return 0;
}

extern "C" int uq_qc_accumulate(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                                uint32_t ncycles, uint64_t* d_qc) {
    UQ_REQUIRE(ctx && d_buf && d_line_start && d_qc, "uq_qc_accumulate: null argument");
    UQ_REQUIRE(uq_qc_words(ncycles) != 0, "uq_qc_accumulate: ncycles = %u is outside 1 .. %u", ncycles, (unsigned)UQ_QC_MAX_CYCLES);
    UQ_REQUIRE(((uintptr_t)d_qc & 7) == 0, "uq_qc_accumulate: d_qc must be 8-byte aligned");
    if (nreads == 0) return 0;
    // the grid needs only an upper bound of the group count (groups hold >= 1 record); surplus workgroups exit at once
    const uint32_t blocks = (uint32_t)(nreads < UQ_NUM_CU ? nreads : UQ_NUM_CU);
    qc_kernel<<<blocks, QC_THREADS, 0, ctx->stream>>>(d_buf, d_line_start, first_read, nreads, ncycles, (unsigned long long*)d_qc);
    UQ_LAUNCH_CHECK();
    return 0;
}

// The sequential twin: the definition as it stands, on host memory; needs no GPU.
extern "C" int uq_qc_host(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads, uint32_t ncycles, uint64_t* h_qc) {
    UQ_REQUIRE(h_line_start && h_qc && (h_buf || nreads == 0), "uq_qc_host: null argument");
    UQ_REQUIRE(uq_qc_words(ncycles) != 0, "uq_qc_host: ncycles = %u is outside 1 .. %u", ncycles, (unsigned)UQ_QC_MAX_CYCLES);
    const uint64_t C = ncycles;
    uint64_t* const base = h_qc + qc_off_base(ncycles);
    uint64_t* const qual = h_qc + qc_off_qual(ncycles);
    for (uint64_t i = 0; i < nreads; ++i) {
        const uint64_t* p = h_line_start + 4 * (first_read + i);
        UQ_REQUIRE(p[0] < p[1] && p[1] < p[2] && p[2] < p[3] && p[3] < p[4], "uq_qc_host: record %llu: line starts out of order",
                   (unsigned long long)(first_read + i));
        const uint64_t Ls = p[2] - p[1] - 1, Lu = p[4] - p[3] - 1;
        uint64_t gc = 0, sq = 0;
        for (uint64_t k = 0; k < Ls; ++k) {
            const uint32_t c = qc_cls(h_buf[p[1] + k]);
            gc += c == 1 || c == 2;
            base[(k < C ? k : C) * UQ_QC_NBASE + c] += 1;
        }
        for (uint64_t k = 0; k < Lu; ++k) {
            const uint32_t b = h_buf[p[3] + k], q = qc_phred(b);
            h_qc[3] += b < 33 || b > 126;
            sq += q;
            qual[(k < C ? k : C) * UQ_QC_NQUAL + q] += 1;
        }
        h_qc[0] += 1; h_qc[1] += Ls; h_qc[2] += Lu; h_qc[4] += Ls != Lu;
        h_qc[qc_off_len(ncycles) + (Ls < C ? Ls : C)] += 1;
        if (Lu) h_qc[qc_off_mq(ncycles) + sq / Lu] += 1;
        if (Ls) h_qc[qc_off_gc(ncycles) + 100 * gc / Ls] += 1;
    }
    return 0;
}
