// pairs.hip -- paired-end input (`--mate2`, `--interleaved`).  An extension: the reference reads one stream.
//
// uq_interleave_records merges two FASTQ texts in HBM, record by record, into one: A(first) B(first) A(first + 1) B(first + 1) ...  No scan is
// needed: the record indexes hold the prefix sums.  With base = ls_a[4 first] + ls_b[4 first], A(r) lands at ls_a[4r] + ls_b[4r] - base and
// B(r) at ls_a[4r + 4] + ls_b[4r] - base.  The kernel is built from the destination: the output is cut into tiles of PR_TILE bytes at
// 16-byte-aligned ADDRESSES (the buffer itself may start anywhere), one workgroup per tile.  pairs_origin_kernel, queued in front, leaves
// for every tile the first pair that touches it (one binary search per tile over the monotone ls_a[4r] + ls_b[4r]); the workgroup loads the
// record starts of its pairs into LDS (two segments per pair; segment s begins at s_a[(s + 1) / 2] + s_b[s / 2]), and an item is one
// aligned output vector: lane i takes the vectors i, i + 256, ... of the tile, finds the segment of each by a binary search in LDS, and
//   - a vector that lies inside one segment is one unaligned 16-byte global load and one aligned 16-byte store (global loads do not care
//     about alignment, 16-byte stores at odd addresses do: DESIGN.md section 9);
//   - a vector that crosses ONE segment boundary is two such loads, one inside either segment, shifted together in registers;
//   - a vector with three segments, or with a segment shorter than 16 bytes (records can be 9 bytes long), is put together byte by byte;
//   - the output's first and last vector store only their bytes inside [0, size), byte by byte.
// A lane asks for the vectors of all its PR_UNROLL items before it stores the first.  A 70 kbp record is some 4 400 items like any others.
// Nothing outside [0, size) of the output is written, and nothing outside the records [first, first + n) is read.
// Algorithmic HBM bytes: the text once in and once out + 2 x 32 B of index sectors per pair.
//
// uq_mate_check compares the QNAME lines of pair i (record first_a + i step_a of a, first_b + i step_b of b) by the rule in
// include/uqhip.h: one lane per pair, 8-byte unaligned loads inside the two lines, nothing written but the report.
#include "common.h"

namespace {
constexpr int PR_THREADS = 256;
constexpr uint32_t PR_UNROLL = 4;                               // 16-byte vectors a lane has in flight
constexpr uint32_t PR_TILE = PR_THREADS * PR_UNROLL * 16;       // bytes of output per tile (tests/test_gpu_pairs.py builds its inputs from this)
constexpr uint32_t PR_NP = PR_TILE / 8 + 3;                     // record starts a tile can need: a pair is >= 8 bytes (2 x 4 newlines), + the pair that begins in front + the end
constexpr uint32_t PR_BLOCKS_PER_CU = 4;                        // what 2 x 8 x PR_NP bytes of LDS admit
constexpr int MC_THREADS = 256;
constexpr uint32_t MC_BLOCKS_PER_CU = 8;

// output offset of the first byte tile t may write (tile t's first vector begins mis bytes in front of offset t * PR_TILE)
__device__ __forceinline__ uint64_t pr_tile_lo(uint64_t t, uint32_t mis, uint64_t size) {
    if (t == 0) return 0;
    const uint64_t o = t * PR_TILE - mis;
    return o < size ? o : size;
}

// origin[t] = the last pair r in [first, first + n) with ls_a[4r] + ls_b[4r] - base <= pr_tile_lo(t), for t in [0, ntiles]
__global__ __launch_bounds__(256) void pairs_origin_kernel(const uint64_t* __restrict__ ls_a, const uint64_t* __restrict__ ls_b, uint64_t first, uint64_t n,
                                                           uint64_t base, uint64_t size, uint32_t mis, uint64_t ntiles, uint64_t* __restrict__ origin) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > ntiles) return;
    const uint64_t x = base + pr_tile_lo(t, mis, size);
    uint64_t lo = first, hi = first + n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (ls_a[4 * mid] + ls_b[4 * mid] <= x) lo = mid; else hi = mid;
    }
    origin[t] = lo;
}

// (b is addressed as a + b_minus_a: one base pointer, never one picked between two, so that the accesses stay global, not flat)
__global__ __launch_bounds__(PR_THREADS, PR_BLOCKS_PER_CU) void interleave_kernel(const uint8_t* __restrict__ a, int64_t b_minus_a, const uint64_t* __restrict__ ls_a,
                                                                                   const uint64_t* __restrict__ ls_b, uint64_t end_pair, uint64_t base, uint64_t size,
                                                                                   uint8_t* __restrict__ out, const uint64_t* __restrict__ origin) {
    __shared__ uint64_t s_a[PR_NP], s_b[PR_NP];                 // starts of the records R0 + j of a and of b (offsets in their buffers)
    const uint32_t tid = threadIdx.x;
    const uint64_t t = blockIdx.x;
    const uint32_t mis = (uint32_t)((uintptr_t)out & 15u);
    const int64_t t0 = (int64_t)(t * PR_TILE) - (int64_t)mis;   // output offset of the tile's first vector (negative in tile 0 of a misaligned buffer)
    const uint64_t R0 = origin[t];
    uint64_t last = origin[t + 1] + 1;                          // the record behind the last pair that can begin inside the tile: it closes that pair's B segment
    if (last > end_pair) last = end_pair;
    uint64_t cnt64 = last - R0 + 1;
    const uint32_t cnt = (uint32_t)(cnt64 < PR_NP ? cnt64 : PR_NP);
    for (uint32_t j = tid; j < cnt; j += PR_THREADS) { s_a[j] = ls_a[4 * (R0 + j)]; s_b[j] = ls_b[4 * (R0 + j)]; }
    __syncthreads();
    const uint32_t nseg = 2 * (cnt - 1);                        // segment s, s < nseg, covers the output offsets [start(s), start(s + 1))
    auto start = [&](uint32_t s) { return s_a[(s + 1) >> 1] + s_b[s >> 1] - base; };
    // where the bytes of segment s come from: the byte at output offset d is a[src(s) + d - start(s)]
    auto src = [&](uint32_t s) { return (s & 1u) ? (int64_t)s_b[s >> 1] + b_minus_a : (int64_t)s_a[s >> 1]; };
    const uint32_t top = nseg > 1 ? 1u << (31 - __clz((int)(nseg - 1))) : 0u;

    // An item's vector is put together from at most two 16-byte windows, both asked for before the first item is stored: window A lies
    // inside the segment of the vector's first byte (at that byte, or -- at the segment's end -- ending with the segment, and shifted
    // down), window B is the first 16 bytes of the next segment, shifted up to the boundary.  No window leaves its segment, so nothing
    // outside the records is read.  Segments shorter than 16 bytes, and vectors with three segments, are read byte by byte (kind 2).
    typedef unsigned __int128 u128;
    uint4 va[PR_UNROLL], vb[PR_UNROLL];
    uint32_t meta[PR_UNROLL], seg[PR_UNROLL];                   // meta: kind (0 nothing, 1 windows, 2 bytes) | shift of A << 4 | bytes of A << 9 | place of B << 14 (0: none)
#pragma unroll
    for (uint32_t u = 0; u < PR_UNROLL; ++u) {
        const int64_t o = t0 + 16 * (int64_t)(u * PR_THREADS + tid);
        meta[u] = 0; seg[u] = 0; va[u] = make_uint4(0, 0, 0, 0); vb[u] = make_uint4(0, 0, 0, 0);
        if (o + 16 <= 0 || o >= (int64_t)size || nseg == 0) continue;
        const uint64_t x = o < 0 ? 0 : (uint64_t)o;
        const uint64_t vend = (uint64_t)(o + 16) < size ? (uint64_t)(o + 16) : size;
        uint32_t s = 0;                                         // the last segment that begins at x or in front of it
        for (uint32_t st = top; st; st >>= 1) s += (s + st < nseg && start(s + st) <= x) ? st : 0;
        seg[u] = s;
        const uint64_t b = start(s), e = start(s + 1);
        const uint64_t dhi = vend < e ? vend : e;
        uint32_t kind = 1, sh = 0, place = 0;
        int64_t w = 0;
        if (e - b < 16) kind = 2;
        else {
            const int64_t from = src(s), qs = from + (int64_t)(x - b), wmax = from + (int64_t)(e - b - 16);
            w = qs < wmax ? qs : wmax;
            sh = (uint32_t)(qs - w);
        }
        if (dhi < vend) {                                       // the vector goes on into segment s + 1
            if (s + 1 >= nseg) kind = 2;
            else {
                const uint64_t e2 = start(s + 2);
                if (e2 < vend || e2 - e < 16) kind = 2; else place = (uint32_t)((int64_t)e - o);      // 1 .. 15
            }
        }
        meta[u] = kind | (sh << 4) | ((uint32_t)(dhi - x) << 9) | (place << 14);
        if (kind == 1) {
            __builtin_memcpy(&va[u], a + w, 16);
            if (place) __builtin_memcpy(&vb[u], a + src(s + 1), 16);
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < PR_UNROLL; ++u) {
        const int64_t o = t0 + 16 * (int64_t)(u * PR_THREADS + tid);
        const uint32_t kind = meta[u] & 3u;
        if (kind == 0) continue;
        const uint32_t klo = o < 0 ? (uint32_t)(-o) : 0u;
        const uint32_t khi = (uint64_t)(o + 16) > size ? (uint32_t)((int64_t)size - o) : 16u;
        uint4 r;
        if (kind == 1) {
            const uint32_t sh = (meta[u] >> 4) & 31u, len = (meta[u] >> 9) & 31u, place = (meta[u] >> 14) & 31u;
            u128 A, B;
            __builtin_memcpy(&A, &va[u], 16); __builtin_memcpy(&B, &vb[u], 16);
            A >>= 8 * sh;
            if (len < 16) A &= ((u128)1 << (8 * len)) - 1;
            A <<= 8 * klo;
            if (place) A |= B << (8 * place);
            __builtin_memcpy(&r, &A, 16);
        } else {
            uint32_t s = seg[u];
            uint64_t b = start(s), e = start(s + 1);
            int64_t from = src(s);
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                if (k < klo || k >= khi) continue;
                const uint64_t d = (uint64_t)(o + (int64_t)k);
                while (d >= e && s + 1 < nseg) { ++s; b = e; e = start(s + 1); from = src(s); }
                w[k >> 2] |= (uint32_t)a[from + (int64_t)(d - b)] << (8 * (k & 3u));
            }
            r = make_uint4(w[0], w[1], w[2], w[3]);
        }
        if (klo == 0 && khi == 16) *(uint4*)(out + o) = r;
        else {
            const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k)
                if (k >= klo && k < khi) out[o + (int64_t)k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3u)));
        }
    }
}

// ---- the mate rule
__device__ __forceinline__ uint64_t mc_load8(const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
// high bit of byte k set if byte k of v is c (exact below and at the first such byte)
__device__ __forceinline__ uint64_t mc_eq_bits(uint64_t v, uint8_t c) {
    const uint64_t x = v ^ (0x0101010101010101ull * c);
    return (x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull;
}
// bytes of the line p[0, L) in front of its first space or tab
__device__ __forceinline__ uint32_t mc_id_len(const uint8_t* p, uint32_t L) {
    uint32_t k = 0;
    for (; k + 8 <= L; k += 8) {
        const uint64_t v = mc_load8(p + k);
        const uint64_t m = mc_eq_bits(v, ' ') | mc_eq_bits(v, '\t');
        if (m) return k + ((uint32_t)__builtin_ctzll(m) >> 3);
    }
    for (; k < L; ++k)
        if (p[k] == ' ' || p[k] == '\t') break;
    return k;
}

__global__ __launch_bounds__(MC_THREADS) void mate_check_kernel(const uint8_t* __restrict__ a, const uint64_t* __restrict__ ls_a, uint64_t first_a, uint64_t step_a,
                                                                const uint8_t* __restrict__ b, const uint64_t* __restrict__ ls_b, uint64_t first_b, uint64_t step_b,
                                                                uint64_t n, uint64_t index_base, unsigned long long* __restrict__ report) {
    uint32_t bad = 0, slash = 0;                                // < 2^32: a lane sees fewer than 2^32 pairs of a grid-stride walk over < 2^64 / 8 records
    uint64_t first_bad = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * MC_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * MC_THREADS) {
        const uint64_t* pa = ls_a + 4 * (first_a + i * step_a);
        const uint64_t* pb = ls_b + 4 * (first_b + i * step_b);
        const uint64_t sa = pa[0], sb = pb[0];
        const uint32_t La = (uint32_t)(pa[1] - sa - 1), Lb = (uint32_t)(pb[1] - sb - 1);      // without the newline
        const uint8_t* qa = a + sa;
        const uint8_t* qb = b + sb;
        uint32_t ia = mc_id_len(qa, La), ib = mc_id_len(qb, Lb);
        if (ia >= 2 && ib >= 2 && qa[ia - 2] == '/' && qa[ia - 1] == '1' && qb[ib - 2] == '/' && qb[ib - 1] == '2') { ia -= 2; ib -= 2; ++slash; }
        bool same = ia == ib;
        if (same) {
            uint32_t k = 0;
            for (; k + 8 <= ia; k += 8)
                if (mc_load8(qa + k) != mc_load8(qb + k)) { same = false; break; }
            if (same)
                for (; k < ia; ++k)
                    if (qa[k] != qb[k]) { same = false; break; }
        }
        if (!same) { ++bad; if (first_bad == ~0ull) first_bad = index_base + i; }
    }
    const uint32_t wbad = wave_sum(bad), wslash = wave_sum(slash);
    const uint64_t wfirst = wave_min(first_bad);
    if (lane_id() == 0) {
        if (wbad) { atomicAdd(report + 1, (unsigned long long)wbad); atomicMin(report + 2, (unsigned long long)wfirst); }
        if (wslash) atomicAdd(report + 3, (unsigned long long)wslash);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(report, (unsigned long long)n);
}

// the same rule on host memory, byte by byte
bool mate_rule_host(const uint8_t* qa, uint64_t La, const uint8_t* qb, uint64_t Lb, bool* slash) {
    uint64_t ia = 0, ib = 0;
    while (ia < La && qa[ia] != ' ' && qa[ia] != '\t') ++ia;
    while (ib < Lb && qb[ib] != ' ' && qb[ib] != '\t') ++ib;
    *slash = ia >= 2 && ib >= 2 && qa[ia - 2] == '/' && qa[ia - 1] == '1' && qb[ib - 2] == '/' && qb[ib - 1] == '2';
    if (*slash) { ia -= 2; ib -= 2; }
    return ia == ib && memcmp(qa, qb, ia) == 0;
}
}  // namespace

extern "C" int uq_interleave_records(uq_ctx* ctx, const uint8_t* d_a, const uint64_t* d_ls_a, const uint8_t* d_b, const uint64_t* d_ls_b,
                                     uint64_t first_pair, uint64_t npairs, uint8_t* d_out, uint64_t out_capacity) {
    UQ_REQUIRE(ctx && d_ls_a && d_ls_b, "uq_interleave_records: null argument");
    if (npairs == 0) return 0;
    UQ_REQUIRE(d_a && d_b, "uq_interleave_records: null argument");
    UQ_REQUIRE(first_pair + npairs >= first_pair && first_pair + npairs < (1ull << 59), "uq_interleave_records: records beyond any index");
    // the four record starts that give the output's size: nothing is launched on the buffers before the capacity has been checked
    uint64_t* h = ctx->h_pinned;
    UQ_TRY(uq_read_back(ctx, h + 0, d_ls_a + 4 * first_pair, 8));
    UQ_TRY(uq_read_back(ctx, h + 1, d_ls_a + 4 * (first_pair + npairs), 8));
    UQ_TRY(uq_read_back(ctx, h + 2, d_ls_b + 4 * first_pair, 8));
    UQ_TRY(uq_read_back(ctx, h + 3, d_ls_b + 4 * (first_pair + npairs), 8));
    UQ_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    const uint64_t a0 = h[0], a1 = h[1], b0 = h[2], b1 = h[3];
    UQ_REQUIRE(a1 >= a0 + 4 * npairs && b1 >= b0 + 4 * npairs, "uq_interleave_records: record starts out of order");
    const uint64_t size = (a1 - a0) + (b1 - b0);
    UQ_REQUIRE(out_capacity >= size, "uq_interleave_records: the output needs %llu bytes, out_capacity is %llu", (unsigned long long)size,
               (unsigned long long)out_capacity);
    UQ_REQUIRE(d_out, "uq_interleave_records: null argument");
    const uint32_t mis = (uint32_t)((uintptr_t)d_out & 15u);
    const uint64_t ntiles = (size + mis + PR_TILE - 1) / PR_TILE;
    UQ_REQUIRE(ntiles < (1ull << 31), "uq_interleave_records: more than 2^31 output tiles");
    void* ws;
    UQ_TRY(uq_scratch(ctx, (ntiles + 1) * 8, &ws));
    pairs_origin_kernel<<<(uint32_t)((ntiles + 1 + 255) / 256), 256, 0, ctx->stream>>>(d_ls_a, d_ls_b, first_pair, npairs, a0 + b0, size, mis, ntiles, (uint64_t*)ws);
    UQ_LAUNCH_CHECK();
    interleave_kernel<<<(uint32_t)ntiles, PR_THREADS, 0, ctx->stream>>>(d_a, (int64_t)((uintptr_t)d_b - (uintptr_t)d_a), d_ls_a, d_ls_b, first_pair + npairs,
                                                                        a0 + b0, size, d_out, (const uint64_t*)ws);
    UQ_LAUNCH_CHECK();
    return 0;
}

// The sequential twin: the definition as it stands, on host memory; needs no GPU.
extern "C" int uq_interleave_records_host(const uint8_t* h_a, const uint64_t* h_ls_a, const uint8_t* h_b, const uint64_t* h_ls_b,
                                          uint64_t first_pair, uint64_t npairs, uint8_t* h_out, uint64_t out_capacity) {
    UQ_REQUIRE(h_ls_a && h_ls_b, "uq_interleave_records_host: null argument");
    if (npairs == 0) return 0;
    UQ_REQUIRE(h_a && h_b, "uq_interleave_records_host: null argument");
    const uint64_t* pa = h_ls_a + 4 * first_pair;
    const uint64_t* pb = h_ls_b + 4 * first_pair;
    UQ_REQUIRE(pa[4 * npairs] >= pa[0] && pb[4 * npairs] >= pb[0], "uq_interleave_records_host: record starts out of order");
    const uint64_t size = (pa[4 * npairs] - pa[0]) + (pb[4 * npairs] - pb[0]);
    UQ_REQUIRE(out_capacity >= size, "uq_interleave_records_host: the output needs %llu bytes, out_capacity is %llu", (unsigned long long)size,
               (unsigned long long)out_capacity);
    UQ_REQUIRE(h_out, "uq_interleave_records_host: null argument");
    uint64_t at = 0;
    for (uint64_t r = 0; r < npairs; ++r) {
        UQ_REQUIRE(pa[4 * r + 4] >= pa[4 * r] && pb[4 * r + 4] >= pb[4 * r], "uq_interleave_records_host: pair %llu: record starts out of order",
                   (unsigned long long)(first_pair + r));
        memcpy(h_out + at, h_a + pa[4 * r], pa[4 * r + 4] - pa[4 * r]); at += pa[4 * r + 4] - pa[4 * r];
        memcpy(h_out + at, h_b + pb[4 * r], pb[4 * r + 4] - pb[4 * r]); at += pb[4 * r + 4] - pb[4 * r];
    }
    return 0;
}

extern "C" int uq_mate_report_init(uq_ctx* ctx, uq_mate_report* d_report) {
    UQ_REQUIRE(ctx && d_report, "uq_mate_report_init: null argument");
    UQ_CHECK_HIP(hipMemsetAsync(d_report, 0, sizeof(uq_mate_report), ctx->stream));
    UQ_CHECK_HIP(hipMemsetAsync(&d_report->first_mismatch, 0xFF, 8, ctx->stream));
    return 0;
}

extern "C" int uq_mate_check(uq_ctx* ctx, const uint8_t* d_a, const uint64_t* d_ls_a, uint64_t first_a, uint64_t step_a,
                             const uint8_t* d_b, const uint64_t* d_ls_b, uint64_t first_b, uint64_t step_b,
                             uint64_t npairs, uint64_t pair_index_base, uq_mate_report* d_report) {
    UQ_REQUIRE(ctx && d_ls_a && d_ls_b && d_report, "uq_mate_check: null argument");
    UQ_REQUIRE(((uintptr_t)d_report & 7) == 0, "uq_mate_check: d_report must be 8-byte aligned");
    if (npairs == 0) return 0;
    UQ_REQUIRE(d_a && d_b, "uq_mate_check: null argument");
    const uint64_t want = (npairs + MC_THREADS - 1) / MC_THREADS;
    const uint32_t blocks = (uint32_t)(want < UQ_NUM_CU * MC_BLOCKS_PER_CU ? want : UQ_NUM_CU * MC_BLOCKS_PER_CU);
    mate_check_kernel<<<blocks, MC_THREADS, 0, ctx->stream>>>(d_a, d_ls_a, first_a, step_a, d_b, d_ls_b, first_b, step_b, npairs, pair_index_base,
                                                              (unsigned long long*)d_report);
    UQ_LAUNCH_CHECK();
    return 0;
}

extern "C" int uq_mate_check_host(const uint8_t* h_a, const uint64_t* h_ls_a, uint64_t first_a, uint64_t step_a,
                                  const uint8_t* h_b, const uint64_t* h_ls_b, uint64_t first_b, uint64_t step_b,
                                  uint64_t npairs, uint64_t pair_index_base, uq_mate_report* h_report) {
    UQ_REQUIRE(h_ls_a && h_ls_b && h_report, "uq_mate_check_host: null argument");
    if (npairs == 0) return 0;
    UQ_REQUIRE(h_a && h_b, "uq_mate_check_host: null argument");
    for (uint64_t i = 0; i < npairs; ++i) {
        const uint64_t* pa = h_ls_a + 4 * (first_a + i * step_a);
        const uint64_t* pb = h_ls_b + 4 * (first_b + i * step_b);
        UQ_REQUIRE(pa[1] > pa[0] && pb[1] > pb[0], "uq_mate_check_host: pair %llu: line starts out of order", (unsigned long long)(pair_index_base + i));
        bool slash;
        const bool same = mate_rule_host(h_a + pa[0], pa[1] - pa[0] - 1, h_b + pb[0], pb[1] - pb[0] - 1, &slash);
        h_report->slash_pairs += slash;
        if (!same) {
            h_report->mismatches += 1;
            if (pair_index_base + i < h_report->first_mismatch) h_report->first_mismatch = pair_index_base + i;
        }
    }
    h_report->pairs += npairs;
    return 0;
}
