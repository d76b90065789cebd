// dedup.hip -- duplicate removal (`--dedup`).  An extension: the reference stores every read it is given.
//
// uq_dedup_keys gives every unit (a record, or an interleaved pair) a 16-byte sort key made from the seeded hash of its compared text (the
// definition is in include/uqhip.h).  dedup_keys_kernel is built like filter_mark_kernel (filter.hip; the stager is copied, not shared:
// DESIGN.md section 27): persistent workgroups walk tiles of R consecutive records (R even under unit 2, so a pair never straddles two tiles),
// a tile is one contiguous span copied to LDS with coalesced 16-byte loads (the next tile's bytes are in flight, its bounds were asked for a turn
// earlier), P lanes (a power of two, 4 .. 16) share a record and take one 8-byte hash word of its sequence per step, acc is reduced over the
// P lanes with shuffles, the mate's hash comes over with one more shuffle, and one lane per unit writes the key row as one 16-byte store.
// Without UQ_DEDUP_BEST the quality line is not touched after staging; with it (the second instantiation) the lanes also take filter.hip's SWAR
// Phred sum of the quality line.  A tile whose span does not fit the stage is read straight from HBM: its records take a half-wave each,
// eight at a time, except those with a line beyond DK_LONG bytes, which the whole workgroup walks -- never one thread along a line; the
// records' hashes meet in LDS and one lane per unit writes the row.
// Algorithmic HBM bytes: the record bytes once + 32 B of line starts per record + 16 B out per unit.
//
// uq_dedup_mark walks the sorted order.  dedup_mark_kernel: a workgroup takes 256 consecutive positions, a lane reads its position's entry of
// the order (coalesced) and the 8 hash bytes of that key (the one gather), neighbours meet in LDS.  A position whose hash differs from its
// predecessor's opens a class and is done; the others -- the duplicates, and the rare collisions -- are listed in LDS and taken by groups of
// DM_GROUP lanes, which compare the two units with 16-byte loads straight from HBM, a loop along long lines.  So the text traffic scales with the
// number of hash-equal neighbours and with nothing else; no workgroup waits for another; the counters go through LDS, one atomic per field
// per workgroup.  The verdicts are cleared by one fill in front of the kernel, which then writes the duplicates' bytes only.
#include "common.h"
#include "swar.h"
#include <stdlib.h>

namespace {
constexpr uint64_t DD_K = 0x9E3779B97F4A7C15ull;
__host__ __device__ __forceinline__ uint64_t dd_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
enum { DR_READS_IN = 0, DR_BASES_IN, DR_UNITS_IN, DR_CLASSES, DR_DUP_UNITS, DR_DUP_READS, DR_DUP_BASES, DR_COLLISIONS, DR_WORDS };
static_assert(sizeof(uq_dedup_report) == DR_WORDS * 8, "the report is eight u64 words");
static_assert(sizeof(uq_dedup_params) == 24, "the parameters are four u32 and one u64");

// the definition's pieces (the one place they are written: kernels and host twins)
__host__ __device__ __forceinline__ uint64_t dd_word(uint64_t w, uint64_t k, uint64_t S) { return dd_mix((w ^ S) + DD_K * (k + 1)); }
__host__ __device__ __forceinline__ uint64_t dd_close(uint64_t acc, uint64_t Lc) { return dd_mix(acc + DD_K * Lc + 2); }
__host__ __device__ __forceinline__ uint64_t dd_clip(uint64_t Ls, uint32_t prefix) { return prefix != 0 && prefix < Ls ? prefix : Ls; }
__host__ __device__ __forceinline__ uint32_t dd_bswap(uint32_t v) { return __builtin_bswap32(v); }

struct DdArgs { uint64_t S, mask, unit_base; uint32_t prefix, unit; };      // S = mix(seed + K); mask = the low hash_bits; unit_base = the first unit's number

// the key row of unit w: H, 0xFFFFFFFF - score (0 without BEST), w, each big-endian
template <bool BEST>
__host__ __device__ __forceinline__ uint4 dd_key(uint64_t H, uint64_t score, uint64_t w) {
    const uint32_t sc = score > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)score;
    return make_uint4(dd_bswap((uint32_t)(H >> 32)), dd_bswap((uint32_t)H), BEST ? dd_bswap(0xFFFFFFFFu - sc) : 0u, dd_bswap((uint32_t)w));
}
__host__ __device__ __forceinline__ uint64_t dd_unit_hash(const DdArgs& a, uint64_t d1, uint64_t d2) {
    return (a.unit == 2 ? dd_mix(d1 + dd_mix(d2)) : d1) & a.mask;
}

// ---- the keys
constexpr int DK_THREADS = 256;
constexpr int DK_NV = 5;                          // 16-byte loads per lane per tile
constexpr uint32_t DK_CAP = DK_NV * 256 * 16;     // staging bytes per tile (20 KiB)
constexpr uint32_t DK_RMAX = 64;                  // records per tile, upper bound (4 * DK_RMAX + 1 <= 2 * DK_THREADS)
constexpr uint64_t DK_LONG = 4096;                // in a tile beyond the stage: a line longer than this is walked by the whole workgroup, the others by a half-wave

typedef unsigned short dk_us2 __attribute__((ext_vector_type(2)));
// SUM of clamp(b, 33, 126) over the four bytes of w (filter.hip's SWAR clamp)
__device__ __forceinline__ uint32_t dk_clamped_sum4(uint32_t w) {
    const uint32_t ev = w & 0x00FF00FFu, od = (w >> 8) & 0x00FF00FFu;
    dk_us2 a, b;
    __builtin_memcpy(&a, &ev, 4); __builtin_memcpy(&b, &od, 4);
    const dk_us2 lo = {33, 33}, hi = {126, 126};
    a = __builtin_elementwise_min(__builtin_elementwise_max(a, lo), hi);
    b = __builtin_elementwise_min(__builtin_elementwise_max(b, lo), hi);
    a += b;
    return (uint32_t)a.x + (uint32_t)a.y;
}
__device__ __forceinline__ uint32_t dk_qsum4(uint32_t w) { return dk_clamped_sum4(w) - 4u * 33u; }
// the Phred sum of the bytes k < cnt of an 8-byte window: bytes beyond the line become '!' (quality 0)
__device__ __forceinline__ uint32_t dk_phred_sum8(uint32_t lo, uint32_t hi, uint32_t cnt) {
    const uint32_t nlo = cnt < 4 ? cnt : 4u, nhi = cnt < 8 ? cnt - nlo : 4u;
    const uint32_t klo = nlo == 4 ? 0xFFFFFFFFu : (1u << (8 * nlo)) - 1u, khi = nhi == 4 ? 0xFFFFFFFFu : (1u << (8 * nhi)) - 1u;
    return dk_qsum4(bfi(klo, lo, 0x21212121u)) + dk_qsum4(bfi(khi, hi, 0x21212121u));
}
// the hash word of the bytes k < cnt of an 8-byte window: the bytes beyond the text are zero
__device__ __forceinline__ uint64_t dk_word8(uint32_t lo, uint32_t hi, uint32_t cnt) {
    if (cnt < 4) { lo &= (1u << (8 * cnt)) - 1u; hi = 0; }
    else if (cnt < 8) hi &= (1u << (8 * (cnt - 4))) - 1u;
    return (uint64_t)lo | ((uint64_t)hi << 32);
}
// one text b[0, L) in HBM walked by `nl` lanes, this one being lane `l` of them, 16 bytes (two hash words) a step inside the text: its share of acc
__device__ __forceinline__ uint64_t dk_line_hash(const uint8_t* b, uint64_t L, uint32_t l, uint32_t nl, uint64_t S) {
    uint64_t acc = 0;
    for (uint64_t j = 16ull * l; j < L; j += 16ull * nl) {
        uint64_t w0 = 0, w1 = 0;
        if (j + 16 <= L) {
            uint4 v;
            __builtin_memcpy(&v, b + j, 16);
            w0 = (uint64_t)v.x | ((uint64_t)v.y << 32); w1 = (uint64_t)v.z | ((uint64_t)v.w << 32);
        } else {
            for (uint64_t k = j; k < L; ++k) {
                const uint64_t byte = b[k];
                if (k - j < 8) w0 |= byte << (8 * (k - j)); else w1 |= byte << (8 * (k - j - 8));
            }
        }
        acc += dd_word(w0, j >> 3, S);
        if (j + 8 < L) acc += dd_word(w1, (j >> 3) + 1, S);
    }
    return acc;
}
__device__ __forceinline__ uint64_t dk_line_q(const uint8_t* b, uint64_t L, uint32_t l, uint32_t nl) {
    uint64_t c = 0;
    for (uint64_t j = 16ull * l; j < L; j += 16ull * nl) {
        if (j + 16 <= L) {
            uint4 w;
            __builtin_memcpy(&w, b + j, 16);
            c += dk_qsum4(w.x) + dk_qsum4(w.y) + dk_qsum4(w.z) + dk_qsum4(w.w);
        } else {
            for (uint64_t k = j; k < L; ++k) { const uint32_t ch = b[k]; c += (ch < 33u ? 33u : (ch > 126u ? 126u : ch)) - 33u; }
        }
    }
    return c;
}

template <bool BEST>
__global__ __launch_bounds__(DK_THREADS) void dedup_keys_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ ls, uint64_t first, uint64_t n,
                                                                DdArgs arg, uint4* __restrict__ keys, unsigned long long* __restrict__ report) {
    __shared__ __align__(16) uint8_t stage[DK_CAP + 32];
    __shared__ uint32_t meta[4 * DK_RMAX + 4];
    __shared__ uint32_t cfg[2];
    __shared__ uint64_t red[DK_THREADS / 64][2];
    __shared__ uint64_t rec_dl[DK_RMAX], rec_q[DK_RMAX];           // a tile beyond the stage: the records' hashes and Phred sums meet here
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const uint32_t unit = arg.unit, prefix = arg.prefix;
    const uint64_t S = arg.S;
    // the tile geometry is decided here from the average record length (no round trip in front of the launch, as in filter.hip)
    if (tid == 0) {
        const uint64_t avg = (ls[4 * (first + n)] - ls[4 * first]) / n + 1;
        uint64_t R = (DK_CAP - 64) / (avg + avg / 8 + 1);
        R = R > DK_RMAX ? DK_RMAX : (R < 1 ? 1 : R);
        if (unit == 2) R = R < 2 ? 2 : (R & ~uint64_t(1));           // whole pairs: n and `first` are even, so every tile starts at a first mate
        uint32_t P = 16;
        while (P > 1 && P * (uint32_t)R > DK_THREADS) P >>= 1;       // a power of two: the lanes of a record reduce with shuffles
        cfg[0] = (uint32_t)R; cfg[1] = P;
    }
    __syncthreads();
    const uint32_t R = __builtin_amdgcn_readfirstlane(cfg[0]), P = __builtin_amdgcn_readfirstlane(cfg[1]);
    const uint64_t ntiles = (n + R - 1) / R;
    const uint32_t rr = tid / P, pp = tid & (P - 1);
    uint64_t bases = 0;

    const uint64_t G = gridDim.x;
    struct Bounds { uint64_t g0, g1; };
    struct Regs { uint4 v[DK_NV]; uint64_t m0, m1; uint64_t g0; uint32_t skew, nvec, Rt; bool exists, staged; };
    auto load_bounds = [&](uint64_t tt) {
        Bounds b{0, 0};
        if (tt < ntiles) {
            const uint32_t Rn = (uint32_t)((n - tt * R) < R ? (n - tt * R) : R);
            b.g0 = ls[4 * (first + tt * R)]; b.g1 = ls[4 * (first + tt * R) + 4 * Rn];
        }
        return b;
    };
    auto issue = [&](uint64_t tt, Bounds b) {
        Regs x;
        x.exists = tt < ntiles; x.staged = false; x.m0 = x.m1 = 0; x.g0 = b.g0; x.skew = 0; x.nvec = 0; x.Rt = 0;
        for (int u = 0; u < DK_NV; ++u) x.v[u] = make_uint4(0, 0, 0, 0);
        if (!x.exists) return x;
        x.Rt = (uint32_t)((n - tt * R) < R ? (n - tt * R) : R);
        const uint64_t a0 = ((uint64_t)(uintptr_t)buf + b.g0) & ~uint64_t(15);
        x.skew = (uint32_t)(((uint64_t)(uintptr_t)buf + b.g0) - a0);
        const uint64_t span = b.g1 - b.g0 + x.skew;
        x.staged = span + 16 <= DK_CAP;
        if (!x.staged) return x;
        x.nvec = (uint32_t)((span + 15) >> 4);
        const uint4* src = (const uint4*)(buf + ((int64_t)b.g0 - (int64_t)x.skew));      // aligned vectors that hold at least one byte of the span
#pragma unroll
        for (int u = 0; u < DK_NV; ++u) { const uint32_t i = u * DK_THREADS + tid; if (i < x.nvec) x.v[u] = src[i]; }
        const uint64_t* lsp = ls + 4 * (first + tt * R);
        if (tid <= 4 * x.Rt) x.m0 = lsp[tid];
        if (tid + DK_THREADS <= 4 * x.Rt) x.m1 = lsp[tid + DK_THREADS];
        return x;
    };

    uint64_t t = blockIdx.x;
    Bounds b_next = load_bounds(t + G);
    Regs cur = issue(t, load_bounds(t));
    for (; t < ntiles; t += G) {
        const uint64_t r0 = t * R;
        const uint32_t Rt = cur.Rt;
        const Bounds b_nn = load_bounds(t + 2 * G);
        if (cur.staged) {
            if (tid <= 4 * Rt) meta[tid] = (uint32_t)(cur.m0 - cur.g0) + cur.skew;
            if (tid + DK_THREADS <= 4 * Rt) meta[tid + DK_THREADS] = (uint32_t)(cur.m1 - cur.g0) + cur.skew;
#pragma unroll
            for (int u = 0; u < DK_NV; ++u) { const uint32_t i = u * DK_THREADS + tid; if (i < cur.nvec) ((uint4*)stage)[i] = cur.v[u]; }
        }
        __syncthreads();
        const bool staged = cur.staged;
        cur = issue(t + G, b_next);          // the next tile's loads fly while this one is hashed
        b_next = b_nn;
        if (staged) {
            uint64_t acc = 0;
            uint32_t qsum = 0, Ls = 0, Lc = 0;                  // a staged line is shorter than the stage: the Phred sum fits 32 bits
            if (rr < Rt) {
                const uint32_t s = meta[4 * rr + 1], e1 = meta[4 * rr + 2];
                Ls = e1 - s - 1; Lc = (uint32_t)dd_clip(Ls, prefix);
                for (uint32_t j = 8 * pp, k = pp; j < Lc; j += 8 * P, k += P) {
                    uint32_t lo, hi;
                    lds_window8(stage, (int32_t)(s + j), lo, hi);
                    acc += dd_word(dk_word8(lo, hi, Lc - j), k, S);
                }
                if (BEST) {
                    const uint32_t q = meta[4 * rr + 3], e2 = meta[4 * rr + 4], Lu = e2 - q - 1;
                    for (uint32_t j = 8 * pp; j < Lu; j += 8 * P) {
                        uint32_t lo, hi;
                        lds_window8(stage, (int32_t)(q + j), lo, hi);
                        qsum += dk_phred_sum8(lo, hi, Lu - j);
                    }
                }
            }
            for (uint32_t d = 1; d < P; d <<= 1) { acc += __shfl_xor(acc, d, 64); if (BEST) qsum += __shfl_xor(qsum, d, 64); }
            const uint64_t dl = dd_close(acc, Lc);
            uint64_t d2 = 0, score = qsum;
            if (unit == 2) {                                    // the second mate's lanes are the next P of the same wave (2 P divides 64, rr is even)
                d2 = __shfl_down(dl, P, 64);
                if (BEST) score += __shfl_down(qsum, P, 64);
            }
            if (rr < Rt && pp == 0) {
                bases += Ls;
                if (unit == 1 || (rr & 1u) == 0) {
                    const uint64_t w = (r0 + rr) / unit;
                    keys[w] = dd_key<BEST>(dd_unit_hash(arg, dl, d2), score, arg.unit_base + w);
                }
            }
        } else {
            // a span beyond the stage (a long read in it, or a run of longer-than-average ones): straight from HBM.  Records whose lines are at
            // most DK_LONG bytes take a half-wave each, eight at a time, with no barrier (as filter.hip does); a record with a longer line is
            // walked by the whole workgroup, 16 bytes a lane inside the line, and reduced over the block.
            const uint64_t* lsp = ls + 4 * (first + r0);
            for (uint32_t rb = 2 * wave; rb < Rt; rb += 2 * (DK_THREADS / 64)) {          // (wave-uniform trips: the shuffles below see whole half-waves)
                const uint32_t r = rb + (lane >> 5), hl = lane & 31u;
                uint64_t Ls = 0, Lc = 0, acc = 0, qsum = 0;
                bool mine = false;
                if (r < Rt) {
                    const uint64_t* p = lsp + 4 * r;
                    const uint64_t s = p[1], e1 = p[2], q = p[3], e2 = p[4];
                    Ls = e1 - s - 1; Lc = dd_clip(Ls, prefix);
                    const uint64_t Lu = e2 - q - 1;
                    mine = Lc <= DK_LONG && (!BEST || Lu <= DK_LONG);
                    if (mine) { acc = dk_line_hash(buf + s, Lc, hl, 32, S); if (BEST) qsum = dk_line_q(buf + q, Lu, hl, 32); }
                }
                for (uint32_t d = 1; d < 32; d <<= 1) { acc += __shfl_xor(acc, d, 64); if (BEST) qsum += __shfl_xor(qsum, d, 64); }
                if (mine && hl == 0) { rec_dl[r] = dd_close(acc, Lc); rec_q[r] = qsum; bases += Ls; }
            }
            for (uint32_t r = 0; r < Rt; ++r) {
                const uint64_t* p = lsp + 4 * r;
                const uint64_t s = p[1], e1 = p[2], q = p[3], e2 = p[4];
                const uint64_t Ls = e1 - s - 1, Lu = e2 - q - 1, Lc = dd_clip(Ls, prefix);
                if (Lc <= DK_LONG && (!BEST || Lu <= DK_LONG)) continue;                   // (the same for every thread: no barrier is skipped by some)
                const uint64_t acc = wave_sum(dk_line_hash(buf + s, Lc, tid, DK_THREADS, S));
                const uint64_t qsum = BEST ? wave_sum(dk_line_q(buf + q, Lu, tid, DK_THREADS)) : 0;
                if (lane == 0) { red[wave][0] = acc; red[wave][1] = qsum; }
                __syncthreads();
                if (tid == 0) {
                    uint64_t a = 0, qs = 0;
                    for (int w = 0; w < DK_THREADS / 64; ++w) { a += red[w][0]; qs += red[w][1]; }
                    rec_dl[r] = dd_close(a, Lc); rec_q[r] = qs; bases += Ls;
                }
                __syncthreads();
            }
            __syncthreads();
            if (tid < Rt / unit) {                              // one lane per unit
                const uint32_t r = tid * unit;
                const uint64_t w = r0 / unit + tid;
                const uint64_t d2 = unit == 2 ? rec_dl[r + 1] : 0, q2 = unit == 2 ? rec_q[r + 1] : 0;
                const uint64_t score = rec_q[r] + q2;           // (lines are shorter than 2^32 bytes: no wrap)
                keys[w] = dd_key<BEST>(dd_unit_hash(arg, rec_dl[r], d2), score, arg.unit_base + w);
            }
        }
        __syncthreads();
    }
    // the report: per-lane sums -> one atomic per field per workgroup
    bases = wave_sum(bases);
    if (lane == 0) red[wave][0] = bases;
    __syncthreads();
    if (tid == 0) {
        uint64_t v = 0;
        for (int w = 0; w < DK_THREADS / 64; ++w) v += red[w][0];
        if (v) atomicAdd(report + DR_BASES_IN, (unsigned long long)v);
        if (blockIdx.x == 0) {
            atomicAdd(report + DR_READS_IN, (unsigned long long)n);
            atomicAdd(report + DR_UNITS_IN, (unsigned long long)(n / unit));
        }
    }
}

// ---- the marks
constexpr int DM_THREADS = 256;
constexpr uint32_t DM_GROUP = 8;                  // lanes that compare one pair of hash-equal neighbours
constexpr uint32_t DM_BLOCKS_PER_CU = 8;

// does a[0, L) differ from b[0, L)?  Walked by `nl` lanes, 16 bytes a step inside the texts; this lane's share
__device__ __forceinline__ uint32_t dm_differs(const uint8_t* a, const uint8_t* b, uint64_t L, uint32_t l, uint32_t nl) {
    for (uint64_t j = 16ull * l; j < L; j += 16ull * nl) {
        if (j + 16 <= L) {
            uint4 x, y;
            __builtin_memcpy(&x, a + j, 16); __builtin_memcpy(&y, b + j, 16);
            if (((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) != 0) return 1u;
        } else {
            for (uint64_t k = j; k < L; ++k) if (a[k] != b[k]) return 1u;
        }
    }
    return 0u;
}

__global__ __launch_bounds__(DM_THREADS) void dedup_mark_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ ls, uint64_t first, uint64_t nunits,
                                                                uint32_t unit, uint32_t prefix, const uint64_t* __restrict__ keys,
                                                                const uint32_t* __restrict__ perm, uint8_t* __restrict__ verdict,
                                                                unsigned long long* __restrict__ report) {
    __shared__ uint64_t s_hash[DM_THREADS + 1];                 // [i + 1]: the hash bytes of the tile's position i; [0]: of the position in front of the tile
    __shared__ uint32_t s_unit[DM_THREADS + 1];                 // the units at those positions
    __shared__ uint32_t s_cand[DM_THREADS];                     // the tile's positions whose hash equals their predecessor's
    __shared__ uint32_t s_ncand;
    __shared__ unsigned long long s_cnt[4];                     // classes, duplicate units, their bases, collisions
    const uint32_t tid = threadIdx.x, lane = lane_id();
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();                                            // (of its own: the counters are zero before any atomic, whatever the grid)
    const uint64_t ntiles = (nunits + DM_THREADS - 1) / DM_THREADS;
    uint32_t opened = 0;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t j = t * DM_THREADS + tid;
        if (tid == 0) s_ncand = 0;
        uint64_t hb = 0;
        if (j < nunits) {
            uint32_t b = perm[j];
            if (b >= nunits) b = 0;                             // (an entry beyond the units reads unit 0, never out of bounds: uq_gather_rows' rule)
            hb = keys[2 * (uint64_t)b];
            s_hash[tid + 1] = hb; s_unit[tid + 1] = b;
            if (tid == 0 && j > 0) {
                uint32_t a = perm[j - 1];
                if (a >= nunits) a = 0;
                s_hash[0] = keys[2 * (uint64_t)a]; s_unit[0] = a;
            }
        }
        __syncthreads();
        if (j < nunits) {
            if (j == 0 || s_hash[tid] != hb) ++opened;
            else s_cand[atomicAdd(&s_ncand, 1u)] = tid;
        }
        __syncthreads();
        const uint32_t nc = s_ncand;
        for (uint32_t base = 0; base < nc; base += DM_THREADS / DM_GROUP) {      // (the same trips for every thread: the shuffles below see whole groups)
            const uint32_t c = base + tid / DM_GROUP, gl = tid & (DM_GROUP - 1);
            const bool valid = c < nc;
            uint32_t diff = 0, b = 0;
            uint64_t dup_bases = 0;
            if (valid) {
                const uint32_t i = s_cand[c], a = s_unit[i];
                b = s_unit[i + 1];
                for (uint32_t m = 0; m < unit; ++m) {
                    const uint64_t* pa = ls + 4 * (first + (uint64_t)a * unit + m);
                    const uint64_t* pb = ls + 4 * (first + (uint64_t)b * unit + m);
                    const uint64_t sa = pa[1], La = pa[2] - sa - 1, sb = pb[1], Lb = pb[2] - sb - 1;
                    const uint64_t Lca = dd_clip(La, prefix), Lcb = dd_clip(Lb, prefix);
                    dup_bases += Lb;
                    if (Lca != Lcb) diff = 1u;
                    else if (!diff) diff = dm_differs(buf + sa, buf + sb, Lca, gl, DM_GROUP);
                }
            }
            for (uint32_t d = 1; d < DM_GROUP; d <<= 1) diff |= __shfl_xor(diff, d, 64);
            if (valid && gl == 0) {
                if (!diff) {
                    for (uint32_t m = 0; m < unit; ++m) verdict[(uint64_t)b * unit + m] = 1;
                    atomicAdd(&s_cnt[1], 1ull); atomicAdd(&s_cnt[2], (unsigned long long)dup_bases);
                } else {
                    atomicAdd(&s_cnt[0], 1ull); atomicAdd(&s_cnt[3], 1ull);
                }
            }
        }
        __syncthreads();
    }
    opened = wave_sum(opened);
    if (lane == 0 && opened) atomicAdd(&s_cnt[0], (unsigned long long)opened);
    __syncthreads();
    if (tid == 0) {
        if (s_cnt[0]) atomicAdd(report + DR_CLASSES, s_cnt[0]);
        if (s_cnt[1]) { atomicAdd(report + DR_DUP_UNITS, s_cnt[1]); atomicAdd(report + DR_DUP_READS, s_cnt[1] * unit); }
        if (s_cnt[2]) atomicAdd(report + DR_DUP_BASES, s_cnt[2]);
        if (s_cnt[3]) atomicAdd(report + DR_COLLISIONS, s_cnt[3]);
    }
}

int dd_check_params(const char* who, const uq_dedup_params* p, uint64_t first_read, uint64_t nreads, uint64_t unit_index_base) {
    UQ_REQUIRE(p, "%s: null argument", who);
    UQ_REQUIRE(p->unit == 1 || p->unit == 2, "%s: unit is %u, not 1 or 2", who, p->unit);
    UQ_REQUIRE(p->unit == 1 || ((nreads | first_read | unit_index_base) & 1) == 0,
               "%s: unit 2 takes whole pairs: nreads %llu, first_read %llu, unit_index_base %llu", who, (unsigned long long)nreads,
               (unsigned long long)first_read, (unsigned long long)unit_index_base);
    UQ_REQUIRE(p->hash_bits >= 1 && p->hash_bits <= 64, "%s: hash_bits %u is outside 1 .. 64", who, p->hash_bits);
    UQ_REQUIRE((p->flags & ~UQ_DEDUP_BEST) == 0, "%s: unknown flag bits %#x", who, p->flags);
    UQ_REQUIRE(first_read + nreads >= first_read && first_read + nreads < (1ull << 59), "%s: records beyond any index", who);
    UQ_REQUIRE(unit_index_base / p->unit <= (1ull << 32) && nreads / p->unit <= (1ull << 32) - unit_index_base / p->unit,
               "%s: more than 2^32 units: unit_index_base %llu, nreads %llu", who, (unsigned long long)unit_index_base, (unsigned long long)nreads);
    return 0;
}

DdArgs dd_args(const uq_dedup_params* p, uint64_t unit_index_base) {
    DdArgs a;
    a.S = dd_mix(p->seed + DD_K);
    a.mask = p->hash_bits == 64 ? ~0ull : (1ull << p->hash_bits) - 1;
    a.unit_base = unit_index_base / p->unit;
    a.prefix = p->prefix; a.unit = p->unit;
    return a;
}

// DL(c) of the text c = h[0, Lc), sequentially
uint64_t dd_line_hash_host(const uint8_t* h, uint64_t Lc, uint64_t S) {
    uint64_t acc = 0;
    for (uint64_t k = 0; 8 * k < Lc; ++k) {
        uint64_t w = 0;
        for (uint64_t i = 8 * k; i < Lc && i < 8 * k + 8; ++i) w |= (uint64_t)h[i] << (8 * (i - 8 * k));
        acc += dd_word(w, k, S);
    }
    return dd_close(acc, Lc);
}
}  // namespace

extern "C" int uq_dedup_report_init(uq_ctx* ctx, uq_dedup_report* d_report) {
    UQ_REQUIRE(ctx && d_report, "uq_dedup_report_init: null argument");
    UQ_CHECK_HIP(hipMemsetAsync(d_report, 0, sizeof(uq_dedup_report), ctx->stream));
    return 0;
}

extern "C" int uq_dedup_report_init_host(uq_dedup_report* h_report) {
    UQ_REQUIRE(h_report, "uq_dedup_report_init_host: null argument");
    memset(h_report, 0, sizeof(uq_dedup_report));
    return 0;
}

extern "C" int uq_dedup_keys(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                             uint64_t unit_index_base, const uq_dedup_params* h_params, uint8_t* d_keys, uq_dedup_report* d_report) {
    UQ_REQUIRE(ctx && d_line_start && d_report, "uq_dedup_keys: null argument");
    UQ_TRY(dd_check_params("uq_dedup_keys", h_params, first_read, nreads, unit_index_base));
    UQ_REQUIRE(((uintptr_t)d_report & 7) == 0, "uq_dedup_keys: d_report must be 8-byte aligned");
    UQ_REQUIRE(((uintptr_t)d_keys & 15) == 0, "uq_dedup_keys: d_keys must be 16-byte aligned");
    if (nreads == 0) return 0;
    UQ_REQUIRE(d_buf && d_keys, "uq_dedup_keys: null argument");
    // an upper bound of the tile count (a tile holds >= 1 record); surplus workgroups leave at once
    const uint32_t blocks = (uint32_t)(nreads < UQ_NUM_CU * 4 ? nreads : UQ_NUM_CU * 4);
    const DdArgs a = dd_args(h_params, unit_index_base);
    if (h_params->flags & UQ_DEDUP_BEST)
        dedup_keys_kernel<true><<<blocks, DK_THREADS, 0, ctx->stream>>>(d_buf, d_line_start, first_read, nreads, a, (uint4*)d_keys, (unsigned long long*)d_report);
    else
        dedup_keys_kernel<false><<<blocks, DK_THREADS, 0, ctx->stream>>>(d_buf, d_line_start, first_read, nreads, a, (uint4*)d_keys, (unsigned long long*)d_report);
    UQ_LAUNCH_CHECK();
    return 0;
}

extern "C" int uq_dedup_mark(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                             uint64_t unit_index_base, const uq_dedup_params* h_params, const uint8_t* d_keys, const uint32_t* d_perm,
                             uint8_t* d_verdict, uq_dedup_report* d_report) {
    UQ_REQUIRE(ctx && d_line_start && d_report, "uq_dedup_mark: null argument");
    UQ_TRY(dd_check_params("uq_dedup_mark", h_params, first_read, nreads, unit_index_base));
    UQ_REQUIRE(((uintptr_t)d_report & 7) == 0, "uq_dedup_mark: d_report must be 8-byte aligned");
    UQ_REQUIRE(((uintptr_t)d_keys & 15) == 0, "uq_dedup_mark: d_keys must be 16-byte aligned");
    UQ_REQUIRE(((uintptr_t)d_perm & 3) == 0, "uq_dedup_mark: d_perm must be 4-byte aligned");
    if (nreads == 0) return 0;
    UQ_REQUIRE(d_buf && d_keys && d_perm && d_verdict, "uq_dedup_mark: null argument");
    const uint64_t nunits = nreads / h_params->unit;
    UQ_CHECK_HIP(hipMemsetAsync(d_verdict, 0, nreads, ctx->stream));      // every record's byte; the kernel writes the duplicates' only
    const uint64_t want = (nunits + DM_THREADS - 1) / DM_THREADS;
    const uint32_t blocks = (uint32_t)(want < UQ_NUM_CU * DM_BLOCKS_PER_CU ? want : UQ_NUM_CU * DM_BLOCKS_PER_CU);
    dedup_mark_kernel<<<blocks, DM_THREADS, 0, ctx->stream>>>(d_buf, d_line_start, first_read, nunits, h_params->unit, h_params->prefix,
                                                              (const uint64_t*)d_keys, d_perm, d_verdict, (unsigned long long*)d_report);
    UQ_LAUNCH_CHECK();
    return 0;
}

extern "C" int uq_dedup_keys_host(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                                  uint64_t unit_index_base, const uq_dedup_params* h_params, uint8_t* h_keys, uq_dedup_report* h_report) {
    UQ_REQUIRE(h_line_start && h_report, "uq_dedup_keys_host: null argument");
    UQ_TRY(dd_check_params("uq_dedup_keys_host", h_params, first_read, nreads, unit_index_base));
    if (nreads == 0) return 0;
    UQ_REQUIRE(h_buf && h_keys, "uq_dedup_keys_host: null argument");
    const DdArgs a = dd_args(h_params, unit_index_base);
    const bool best = (h_params->flags & UQ_DEDUP_BEST) != 0;
    for (uint64_t w = 0; w < nreads / a.unit; ++w) {
        uint64_t d[2] = {0, 0}, score = 0;
        for (uint32_t m = 0; m < a.unit; ++m) {
            const uint64_t* p = h_line_start + 4 * (first_read + w * a.unit + m);
            UQ_REQUIRE(p[1] > p[0] && p[2] > p[1] && p[3] > p[2] && p[4] > p[3], "uq_dedup_keys_host: record %llu: line starts out of order",
                       (unsigned long long)(first_read + w * a.unit + m));
            const uint64_t Ls = p[2] - p[1] - 1, Lu = p[4] - p[3] - 1;
            d[m] = dd_line_hash_host(h_buf + p[1], dd_clip(Ls, a.prefix), a.S);
            if (best)
                for (uint64_t k = 0; k < Lu; ++k) { const uint32_t c = h_buf[p[3] + k]; score += (c < 33u ? 33u : (c > 126u ? 126u : c)) - 33u; }
            h_report->reads_in += 1; h_report->bases_in += Ls;
        }
        const uint4 row = best ? dd_key<true>(dd_unit_hash(a, d[0], d[1]), score, a.unit_base + w) : dd_key<false>(dd_unit_hash(a, d[0], d[1]), score, a.unit_base + w);
        memcpy(h_keys + 16 * w, &row, 16);
        h_report->units_in += 1;
    }
    return 0;
}

extern "C" int uq_dedup_mark_host(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                                  uint64_t unit_index_base, const uq_dedup_params* h_params, const uint8_t* h_keys, const uint32_t* h_perm,
                                  uint8_t* h_verdict, uq_dedup_report* h_report) {
    UQ_REQUIRE(h_line_start && h_report, "uq_dedup_mark_host: null argument");
    UQ_TRY(dd_check_params("uq_dedup_mark_host", h_params, first_read, nreads, unit_index_base));
    if (nreads == 0) return 0;
    UQ_REQUIRE(h_buf && h_keys && h_perm && h_verdict, "uq_dedup_mark_host: null argument");
    const uint32_t unit = h_params->unit, prefix = h_params->prefix;
    const uint64_t nunits = nreads / unit;
    for (uint64_t j = 0; j < nunits; ++j)
        UQ_REQUIRE(h_perm[j] < nunits, "uq_dedup_mark_host: the order's entry %llu is %u, beyond the %llu units", (unsigned long long)j, h_perm[j],
                   (unsigned long long)nunits);
    memset(h_verdict, 0, nreads);
    for (uint64_t j = 0; j < nunits; ++j) {
        const uint64_t b = h_perm[j];
        if (j == 0 || memcmp(h_keys + 16 * (uint64_t)h_perm[j - 1], h_keys + 16 * b, 8) != 0) { h_report->classes += 1; continue; }
        const uint64_t a = h_perm[j - 1];
        bool equal = true;
        uint64_t dup_bases = 0;
        for (uint32_t m = 0; m < unit; ++m) {
            const uint64_t* pa = h_line_start + 4 * (first_read + a * unit + m);
            const uint64_t* pb = h_line_start + 4 * (first_read + b * unit + m);
            const uint64_t La = pa[2] - pa[1] - 1, Lb = pb[2] - pb[1] - 1;
            const uint64_t Lca = dd_clip(La, prefix), Lcb = dd_clip(Lb, prefix);
            dup_bases += Lb;
            equal = equal && Lca == Lcb && memcmp(h_buf + pa[1], h_buf + pb[1], Lca) == 0;
        }
        if (equal) {
            for (uint32_t m = 0; m < unit; ++m) h_verdict[b * unit + m] = 1;
            h_report->dup_units += 1; h_report->dup_reads += unit; h_report->dup_bases += dup_bases;
        } else {
            h_report->classes += 1; h_report->collisions += 1;
        }
    }
    return 0;
}
