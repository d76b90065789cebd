// filter.hip -- read filtering (`--filter`).  An extension: the reference stores every read it is given.
//
// uq_filter_mark gives every record a verdict byte (the definition is in include/uqhip.h).  filter_mark_kernel does the statistics kernel's
// work without its tables and is built like it (stats.hip; the stager is copied, not shared): persistent workgroups walk tiles of R consecutive
// records, a tile is one contiguous span copied to LDS with coalesced 16-byte loads (the next tile's bytes are in flight, its bounds were asked for
// a turn earlier), P lanes (a power of two, 4 .. 16) share a record and take 8 bytes of its sequence and of its quality line per step: the N count
// is a zero-byte test on (w | 0x20) ^ 'n', the Phred sum clamps the bytes as packed 16-bit halves (v_pk_max_u16 / v_pk_min_u16), both are
// reduced over the P lanes with shuffles, lane 0 of the record writes the byte.  A tile whose span does not fit the stage (a 70 kbp read in
// it, or a run of longer-than-average reads: about one tile in a hundred of 36-301 bp reads) is read straight from HBM: its records take a
// half-wave each, eight at a time and without a barrier, except those with a line beyond FM_LONG bytes, which the WHOLE workgroup walks with
// 16-byte loads inside the line and a block reduction -- never one thread along a line.
// The report is kept as per-lane sums: one atomic per field per workgroup at the end.
// Algorithmic HBM bytes: the record bytes once (the stage takes whole records, as stats.hip does) + 32 B of line starts per record + 1 B out.
//
// uq_filter_plan is kernel boundaries only (scan.hip says why): filter_units_kernel writes keep[w] and len[w] (0 for a dropped unit) per unit,
// uq_scan_exclusive_u64 turns keep into slots and len into output offsets, filter_scatter_kernel writes src[slot] / dst[slot] and dst[kept].
//
// uq_compact_records is built from the destination like interleave_kernel (pairs.hip): output tiles of CP_TILE bytes at 16-byte aligned
// ADDRESSES, compact_origin_kernel in front finds each tile's first unit (a binary search over dst), the workgroup loads its units' dst
// (as int32 relative to the tile, saturated: only the tile's first and last unit can reach far) and src - dst (u64: the byte at output offset d
// of unit s is buf[d + delta(s)], exact whatever was saturated) into LDS -- CP_NP entries, a unit is at least 4 bytes -- and an item is one
// aligned output vector put together from at most two clamped 16-byte windows, or byte by byte (pairs.hip has the cases).
#include "common.h"
#include "swar.h"
#include <stdlib.h>

namespace {
constexpr uint64_t FL_K = 0x9E3779B97F4A7C15ull;
__host__ __device__ __forceinline__ uint64_t fl_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
enum { FR_READS_IN = 0, FR_BASES_IN, FR_BYTES_IN, FR_READS_OUT, FR_BASES_OUT, FR_BYTES_OUT, FR_MIN_LEN, FR_MAX_LEN, FR_MAX_N, FR_MEAN_Q, FR_SAMPLE, FR_MATE, FR_WORDS };
static_assert(sizeof(uq_filter_report) == FR_WORDS * 8, "the report is twelve u64 words");

// the verdict of a record from its reductions (the one place the rule is written: kernel and host twin)
__host__ __device__ __forceinline__ uint32_t fl_verdict(const uq_filter_params& p, uint64_t g, uint64_t Ls, uint64_t Lu, uint64_t ncount, uint64_t qsum) {
    uint32_t v = 0;
    if (Ls < p.min_len) v |= 1u;
    if (Ls > p.max_len) v |= 2u;
    if (ncount > p.max_n) v |= 4u;
    if (qsum < (uint64_t)p.min_mean_q * Lu) v |= 8u;
    if ((p.flags & UQ_FILTER_SAMPLE) && fl_mix(p.seed + FL_K * ((p.unit == 2 ? g >> 1 : g) + 1)) >= p.sample_threshold) v |= 16u;
    return v;
}

// ---- the verdicts
constexpr int FM_THREADS = 256;
constexpr int FM_NV = 5;                          // 16-byte loads per lane per tile
constexpr uint32_t FM_CAP = FM_NV * 256 * 16;     // staging bytes per tile (20 KiB)
constexpr uint32_t FM_RMAX = 64;                  // records per tile, upper bound (4 * FM_RMAX + 1 <= 2 * FM_THREADS)
constexpr uint64_t FM_LONG = 4096;                // in a tile beyond the stage: a line longer than this is walked by the whole workgroup, the others by a half-wave

typedef unsigned short fm_us2 __attribute__((ext_vector_type(2)));
// high bit of every byte of w that is 'N' or 'n'
__device__ __forceinline__ uint32_t fm_n_bits(uint32_t w) {
    const uint32_t x = (w | 0x20202020u) ^ 0x6E6E6E6Eu;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
// SUM of clamp(b, 33, 126) over the four bytes of w
__device__ __forceinline__ uint32_t fm_clamped_sum4(uint32_t w) {
    const uint32_t ev = w & 0x00FF00FFu, od = (w >> 8) & 0x00FF00FFu;
    fm_us2 a, b;
    __builtin_memcpy(&a, &ev, 4); __builtin_memcpy(&b, &od, 4);
    const fm_us2 lo = {33, 33}, hi = {126, 126};
    a = __builtin_elementwise_min(__builtin_elementwise_max(a, lo), hi);
    b = __builtin_elementwise_min(__builtin_elementwise_max(b, lo), hi);
    a += b;
    return (uint32_t)a.x + (uint32_t)a.y;
}
// the N count of the bytes k < cnt of an 8-byte window, and their Phred sum
__device__ __forceinline__ uint32_t fm_count_n8(uint32_t lo, uint32_t hi, uint32_t cnt) {
    uint32_t klo, khi;
    const uint32_t nlo = cnt < 4 ? cnt : 4u, nhi = cnt < 8 ? cnt - nlo : 4u;
    klo = nlo == 4 ? 0xFFFFFFFFu : (1u << (8 * nlo)) - 1u; khi = nhi == 4 ? 0xFFFFFFFFu : (1u << (8 * nhi)) - 1u;
    return __popc(fm_n_bits(lo & klo)) + __popc(fm_n_bits(hi & khi));
}
// SUM of q(b) over the four bytes of w: the SWAR clamp, or four reads of the 256-byte LDS table tab[b] = q(b) (UQ_FILTER_CLAMP=lds; DESIGN.md
// section 27 has the two measured side by side)
template <bool LUT>
__device__ __forceinline__ uint32_t fm_qsum4(uint32_t w, const uint8_t* tab) {
    if (LUT) return (uint32_t)tab[w & 255u] + tab[(w >> 8) & 255u] + tab[(w >> 16) & 255u] + tab[w >> 24];
    return fm_clamped_sum4(w) - 4u * 33u;
}
template <bool LUT>
__device__ __forceinline__ uint32_t fm_phred_sum8(uint32_t lo, uint32_t hi, uint32_t cnt, const uint8_t* tab) {
    const uint32_t nlo = cnt < 4 ? cnt : 4u, nhi = cnt < 8 ? cnt - nlo : 4u;
    const uint32_t klo = nlo == 4 ? 0xFFFFFFFFu : (1u << (8 * nlo)) - 1u, khi = nhi == 4 ? 0xFFFFFFFFu : (1u << (8 * nhi)) - 1u;
    // bytes beyond the line become '!' (quality 0)
    return fm_qsum4<LUT>(bfi(klo, lo, 0x21212121u), tab) + fm_qsum4<LUT>(bfi(khi, hi, 0x21212121u), tab);
}
// one line b[0, L) in HBM walked by `nl` lanes, this one being lane `l` of them, 16 bytes a step inside the line: its share of the N count or of the Phred sum
__device__ __forceinline__ uint64_t fm_line_n(const uint8_t* b, uint64_t L, uint32_t l, uint32_t nl) {
    uint64_t c = 0;
    for (uint64_t j = 16ull * l; j < L; j += 16ull * nl) {
        if (j + 16 <= L) {
            uint4 w;
            __builtin_memcpy(&w, b + j, 16);
            c += __popc(fm_n_bits(w.x)) + __popc(fm_n_bits(w.y)) + __popc(fm_n_bits(w.z)) + __popc(fm_n_bits(w.w));
        } else {
            for (uint64_t k = j; k < L; ++k) c += (b[k] | 0x20u) == 'n';
        }
    }
    return c;
}
template <bool LUT>
__device__ __forceinline__ uint64_t fm_line_q(const uint8_t* b, uint64_t L, uint32_t l, uint32_t nl, const uint8_t* tab) {
    uint64_t c = 0;
    for (uint64_t j = 16ull * l; j < L; j += 16ull * nl) {
        if (j + 16 <= L) {
            uint4 w;
            __builtin_memcpy(&w, b + j, 16);
            c += fm_qsum4<LUT>(w.x, tab) + fm_qsum4<LUT>(w.y, tab) + fm_qsum4<LUT>(w.z, tab) + fm_qsum4<LUT>(w.w, tab);
        } else {
            for (uint64_t k = j; k < L; ++k) { const uint32_t ch = b[k]; c += (ch < 33u ? 33u : (ch > 126u ? 126u : ch)) - 33u; }
        }
    }
    return c;
}

struct FmAcc {
    uint64_t reads = 0, bases = 0;
    uint32_t fail[5] = {0, 0, 0, 0, 0};         // < 2^32: a lane sees fewer than 2^32 records
    __device__ __forceinline__ void record(uint32_t v, uint64_t Ls) {
        ++reads; bases += Ls;
#pragma unroll
        for (int k = 0; k < 5; ++k) fail[k] += (v >> k) & 1u;
    }
};

template <bool LUT>
__global__ __launch_bounds__(FM_THREADS) void filter_mark_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ ls, uint64_t first, uint64_t n,
                                                                 uint64_t index_base, uq_filter_params prm, uint8_t* __restrict__ verdict,
                                                                 unsigned long long* __restrict__ report) {
    __shared__ __align__(16) uint8_t stage[FM_CAP + 32];
    __shared__ uint32_t meta[4 * FM_RMAX + 4];
    __shared__ uint32_t cfg[2];
    __shared__ uint64_t red[FM_THREADS / 64][8];
    __shared__ uint8_t qtab[256];
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    if (LUT) qtab[tid] = (uint8_t)((tid < 33u ? 33u : (tid > 126u ? 126u : tid)) - 33u);
    // the tile geometry is decided here from the shard's average record length (no round trip in front of the launch, as in stats.hip)
    if (tid == 0) {
        const uint64_t avg = (ls[4 * (first + n)] - ls[4 * first]) / n + 1;
        uint64_t R = (FM_CAP - 64) / (avg + avg / 8 + 1);
        R = R > FM_RMAX ? FM_RMAX : (R < 1 ? 1 : R);
        uint32_t P = 16;
        while (P > 1 && P * (uint32_t)R > FM_THREADS) P >>= 1;      // a power of two: the lanes of a record reduce with shuffles
        cfg[0] = (uint32_t)R; cfg[1] = P;
    }
    __syncthreads();
    const uint32_t R = __builtin_amdgcn_readfirstlane(cfg[0]), P = __builtin_amdgcn_readfirstlane(cfg[1]);
    const uint64_t ntiles = (n + R - 1) / R;
    const uint32_t rr = tid / P, pp = tid & (P - 1);
    FmAcc acc;

    const uint64_t S = gridDim.x;
    struct Bounds { uint64_t g0, g1; };
    struct Regs { uint4 v[FM_NV]; uint64_t m0, m1; uint64_t g0; uint32_t skew, nvec, Rt; bool exists, staged; };
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
        for (int u = 0; u < FM_NV; ++u) x.v[u] = make_uint4(0, 0, 0, 0);
        if (!x.exists) return x;
        x.Rt = (uint32_t)((n - tt * R) < R ? (n - tt * R) : R);
        const uint64_t a0 = ((uint64_t)(uintptr_t)buf + b.g0) & ~uint64_t(15);
        x.skew = (uint32_t)(((uint64_t)(uintptr_t)buf + b.g0) - a0);
        const uint64_t span = b.g1 - b.g0 + x.skew;
        x.staged = span + 16 <= FM_CAP;
        if (!x.staged) return x;
        x.nvec = (uint32_t)((span + 15) >> 4);
        const uint4* src = (const uint4*)(buf + ((int64_t)b.g0 - (int64_t)x.skew));      // aligned vectors that hold at least one byte of the span
#pragma unroll
        for (int u = 0; u < FM_NV; ++u) { const uint32_t i = u * FM_THREADS + tid; if (i < x.nvec) x.v[u] = src[i]; }
        const uint64_t* lsp = ls + 4 * (first + tt * R);
        if (tid <= 4 * x.Rt) x.m0 = lsp[tid];
        if (tid + FM_THREADS <= 4 * x.Rt) x.m1 = lsp[tid + FM_THREADS];
        return x;
    };

    uint64_t t = blockIdx.x;
    Bounds b_next = load_bounds(t + S);
    Regs cur = issue(t, load_bounds(t));
    for (; t < ntiles; t += S) {
        const uint64_t r0 = t * R;
        const uint32_t Rt = cur.Rt;
        const Bounds b_nn = load_bounds(t + 2 * S);
        if (cur.staged) {
            if (tid <= 4 * Rt) meta[tid] = (uint32_t)(cur.m0 - cur.g0) + cur.skew;
            if (tid + FM_THREADS <= 4 * Rt) meta[tid + FM_THREADS] = (uint32_t)(cur.m1 - cur.g0) + cur.skew;
#pragma unroll
            for (int u = 0; u < FM_NV; ++u) { const uint32_t i = u * FM_THREADS + tid; if (i < cur.nvec) ((uint4*)stage)[i] = cur.v[u]; }
        }
        __syncthreads();
        const bool staged = cur.staged;
        cur = issue(t + S, b_next);          // the next tile's loads fly while this one is judged
        b_next = b_nn;
        if (staged) {
            uint32_t ncount = 0, qsum = 0, Ls = 0, Lu = 0;      // a staged line is shorter than the stage: the sums fit 32 bits
            if (rr < Rt) {
                const uint32_t s = meta[4 * rr + 1], e1 = meta[4 * rr + 2], q = meta[4 * rr + 3], e2 = meta[4 * rr + 4];
                Ls = e1 - s - 1; Lu = e2 - q - 1;
                for (uint32_t j = 8 * pp; j < Ls; j += 8 * P) {
                    uint32_t lo, hi;
                    lds_window8(stage, (int32_t)(s + j), lo, hi);
                    ncount += fm_count_n8(lo, hi, Ls - j);
                }
                for (uint32_t j = 8 * pp; j < Lu; j += 8 * P) {
                    uint32_t lo, hi;
                    lds_window8(stage, (int32_t)(q + j), lo, hi);
                    qsum += fm_phred_sum8<LUT>(lo, hi, Lu - j, qtab);
                }
            }
            for (uint32_t d = 1; d < P; d <<= 1) { ncount += __shfl_xor(ncount, d, 64); qsum += __shfl_xor(qsum, d, 64); }
            if (rr < Rt && pp == 0) {
                const uint32_t v = fl_verdict(prm, index_base + r0 + rr, Ls, Lu, ncount, qsum);
                verdict[r0 + rr] = (uint8_t)v;
                acc.record(v, Ls);
            }
        } else {
            // a span beyond the stage (a long read in it, or a run of longer-than-average ones): straight from HBM.  Records whose two lines
            // are at most FM_LONG bytes take a half-wave each, eight at a time, with no barrier (as stats.hip does); a record with a longer
            // line is walked by the whole workgroup, 16 bytes a lane inside the line, and reduced over the block.
            const uint64_t* lsp = ls + 4 * (first + r0);
            for (uint32_t rb = 2 * wave; rb < Rt; rb += 2 * (FM_THREADS / 64)) {          // (wave-uniform trips: the shuffles below see whole half-waves)
                const uint32_t r = rb + (lane >> 5), hl = lane & 31u;
                uint64_t Ls = 0, Lu = 0, ncount = 0, qsum = 0;
                bool mine = false;
                if (r < Rt) {
                    const uint64_t* p = lsp + 4 * r;
                    const uint64_t s = p[1], e1 = p[2], q = p[3], e2 = p[4];
                    Ls = e1 - s - 1; Lu = e2 - q - 1;
                    mine = Ls <= FM_LONG && Lu <= FM_LONG;
                    if (mine) { ncount = fm_line_n(buf + s, Ls, hl, 32); qsum = fm_line_q<LUT>(buf + q, Lu, hl, 32, qtab); }
                }
                for (uint32_t d = 1; d < 32; d <<= 1) { ncount += __shfl_xor(ncount, d, 64); qsum += __shfl_xor(qsum, d, 64); }
                if (mine && hl == 0) {
                    const uint32_t v = fl_verdict(prm, index_base + r0 + r, Ls, Lu, ncount, qsum);
                    verdict[r0 + r] = (uint8_t)v;
                    acc.record(v, Ls);
                }
            }
            for (uint32_t r = 0; r < Rt; ++r) {
                const uint64_t* p = lsp + 4 * r;
                const uint64_t s = p[1], e1 = p[2], q = p[3], e2 = p[4];
                const uint64_t Ls = e1 - s - 1, Lu = e2 - q - 1;
                if (Ls <= FM_LONG && Lu <= FM_LONG) continue;                               // (the same for every thread: no barrier is skipped by some)
                uint64_t ncount = wave_sum(fm_line_n(buf + s, Ls, tid, FM_THREADS));
                uint64_t qsum = wave_sum(fm_line_q<LUT>(buf + q, Lu, tid, FM_THREADS, qtab));
                if (lane == 0) { red[wave][0] = ncount; red[wave][1] = qsum; }
                __syncthreads();
                if (tid == 0) {
                    uint64_t nc = 0, qs = 0;
                    for (int w = 0; w < FM_THREADS / 64; ++w) { nc += red[w][0]; qs += red[w][1]; }
                    const uint32_t v = fl_verdict(prm, index_base + r0 + r, Ls, Lu, nc, qs);
                    verdict[r0 + r] = (uint8_t)v;
                    acc.record(v, Ls);
                }
                __syncthreads();
            }
        }
        __syncthreads();
    }
    // the report: per-lane sums -> one atomic per field per workgroup
    uint64_t f[7] = {acc.reads, acc.bases, acc.fail[0], acc.fail[1], acc.fail[2], acc.fail[3], acc.fail[4]};
#pragma unroll
    for (int k = 0; k < 7; ++k) { f[k] = wave_sum(f[k]); if (lane == 0) red[wave][k] = f[k]; }
    __syncthreads();
    if (tid < 7) {
        uint64_t v = 0;
        for (int w = 0; w < FM_THREADS / 64; ++w) v += red[w][tid];
        const uint32_t field = tid == 0 ? FR_READS_IN : (tid == 1 ? FR_BASES_IN : FR_MIN_LEN + (tid - 2));
        if (v) atomicAdd(report + field, (unsigned long long)v);
    }
    if (blockIdx.x == 0 && tid == 0) atomicAdd(report + FR_BYTES_IN, (unsigned long long)(ls[4 * (first + n)] - ls[4 * first]));
}

// ---- the plan
constexpr uint32_t FP_BLOCKS_PER_CU = 8;

__global__ __launch_bounds__(256) void filter_units_kernel(const uint64_t* __restrict__ ls, uint64_t first, uint64_t nunits, uint32_t unit,
                                                           const uint8_t* __restrict__ verdict, uint64_t* __restrict__ keep, uint64_t* __restrict__ len,
                                                           unsigned long long* __restrict__ report) {
    uint64_t bases = 0;
    uint32_t mate = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < nunits; w += (uint64_t)gridDim.x * 256) {
        const uint32_t v0 = verdict[w * unit], v1 = unit == 2 ? verdict[w * unit + 1] : 0u;
        const bool k = (v0 | v1) == 0;
        const uint64_t* p = ls + 4 * (first + w * unit);
        keep[w] = k ? 1u : 0u;
        len[w] = k ? p[4 * unit] - p[0] : 0u;
        if (k) { bases += p[2] - p[1] - 1; if (unit == 2) bases += p[6] - p[5] - 1; }
        else if (unit == 2) mate += (v0 == 0) + (v1 == 0);
    }
    bases = wave_sum(bases); mate = wave_sum(mate);
    if (lane_id() == 0) {
        if (bases) atomicAdd(report + FR_BASES_OUT, (unsigned long long)bases);
        if (mate) atomicAdd(report + FR_MATE, (unsigned long long)mate);
    }
}

// slot / off: the exclusive scans of keep / len; tot[0] = the kept units, tot[1] = the output bytes
__global__ __launch_bounds__(256) void filter_scatter_kernel(const uint64_t* __restrict__ ls, uint64_t first, uint64_t nunits, uint32_t unit,
                                                             const uint64_t* __restrict__ slot, const uint64_t* __restrict__ off,
                                                             const uint64_t* __restrict__ tot, uint64_t* __restrict__ src, uint64_t* __restrict__ dst,
                                                             unsigned long long* __restrict__ report) {
    const uint64_t kept = tot[0];
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < nunits; w += (uint64_t)gridDim.x * 256) {
        const uint64_t j = slot[w], jn = w + 1 < nunits ? slot[w + 1] : kept;
        if (jn != j) { src[j] = ls[4 * (first + w * unit)]; dst[j] = off[w]; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        dst[kept] = tot[1];
        atomicAdd(report + FR_READS_OUT, (unsigned long long)(kept * unit));
        atomicAdd(report + FR_BYTES_OUT, (unsigned long long)tot[1]);
    }
}

// ---- the compaction
constexpr int CP_THREADS = 256;
constexpr uint32_t CP_UNROLL = 4;                               // 16-byte vectors a lane has in flight
constexpr uint32_t CP_TILE = CP_THREADS * CP_UNROLL * 16;       // bytes of output per tile, 16 KiB (tests/test_gpu_filter.py builds its inputs from this)
constexpr uint32_t CP_NP = CP_TILE / 4 + 3;                     // unit starts a tile can need: a unit is >= 4 bytes (four newlines), + the unit that begins in front + the end
constexpr uint32_t CP_BLOCKS_PER_CU = 3;                        // what 12 x CP_NP bytes of LDS admit
constexpr int64_t CP_FAR = 1 << 29;                             // where the relative starts saturate: far beyond a tile on either side (2 CP_FAR fits an int32)

__device__ __forceinline__ uint64_t cp_tile_lo(uint64_t t, uint32_t mis, uint64_t size) {
    if (t == 0) return 0;
    const uint64_t o = t * CP_TILE - mis;
    return o < size ? o : size;
}

// the four words uq_compact_records checks before it launches anything on the buffers, gathered for one read-back
__global__ void compact_ends_kernel(const uint64_t* __restrict__ src, const uint64_t* __restrict__ dst, uint64_t kept, uint64_t* __restrict__ out) {
    out[0] = dst[0]; out[1] = dst[kept]; out[2] = dst[kept - 1]; out[3] = src[kept - 1];
}

// origin[t] = the last unit j in [0, kept) with dst[j] <= cp_tile_lo(t), for t in [0, ntiles]
__global__ __launch_bounds__(256) void compact_origin_kernel(const uint64_t* __restrict__ dst, uint64_t kept, uint64_t size, uint32_t mis, uint64_t ntiles,
                                                             uint64_t* __restrict__ origin) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > ntiles) return;
    const uint64_t x = cp_tile_lo(t, mis, size);
    uint64_t lo = 0, hi = kept;
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (dst[mid] <= x) lo = mid; else hi = mid;
    }
    origin[t] = lo;
}

__global__ __launch_bounds__(CP_THREADS, CP_BLOCKS_PER_CU) void compact_kernel(const uint8_t* __restrict__ a, const uint64_t* __restrict__ src,
                                                                                const uint64_t* __restrict__ dst, uint64_t kept, uint64_t size,
                                                                                uint8_t* __restrict__ out, const uint64_t* __restrict__ origin) {
    __shared__ uint64_t s_delta[CP_NP];                         // src - dst of unit U0 + j (mod 2^64)
    __shared__ int32_t s_rel[CP_NP];                            // dst of unit U0 + j relative to the tile's first vector, saturated at +- CP_FAR
    const uint32_t tid = threadIdx.x;
    const uint64_t t = blockIdx.x;
    const uint32_t mis = (uint32_t)((uintptr_t)out & 15u);
    const int64_t t0 = (int64_t)(t * CP_TILE) - (int64_t)mis;   // output offset of the tile's first vector (negative in tile 0 of a misaligned buffer)
    const uint64_t U0 = origin[t];
    uint64_t last = origin[t + 1] + 1;                          // the entry behind the last unit that can begin inside the tile: it closes that unit
    if (last > kept) last = kept;
    const uint64_t cnt64 = last - U0 + 1;
    const uint32_t cnt = (uint32_t)(cnt64 < CP_NP ? cnt64 : CP_NP);
    for (uint32_t j = tid; j < cnt; j += CP_THREADS) {
        const uint64_t d = dst[U0 + j];
        int64_t rel = (int64_t)d - t0;
        rel = rel < -CP_FAR ? -CP_FAR : (rel > CP_FAR ? CP_FAR : rel);
        s_rel[j] = (int32_t)rel;
        if (j + 1 < cnt) s_delta[j] = src[U0 + j] - d;          // (src has no entry behind the last unit)
    }
    __syncthreads();
    const uint32_t nseg = cnt - 1;                              // unit s, s < nseg, covers the relative output offsets [s_rel[s], s_rel[s + 1])
    const uint32_t top = nseg > 1 ? 1u << (31 - __clz((int)(nseg - 1))) : 0u;
    // the output's bounds relative to the tile
    const int32_t rel_lo = t0 < 0 ? (int32_t)(-t0) : 0;
    const int64_t left = (int64_t)size - t0;
    const int32_t rel_hi = left < (int64_t)CP_TILE ? (int32_t)left : (int32_t)CP_TILE;
    const uint8_t* at = a + t0;                                 // the byte at relative offset d of unit s is at[d + s_delta[s]]

    // As in interleave_kernel: window A lies inside the unit of the vector's first byte (at that byte, or ending with the unit and shifted
    // down), window B is the first 16 bytes of the next unit, shifted up to the boundary.  No window leaves its unit.
    typedef unsigned __int128 u128;
    uint4 va[CP_UNROLL], vb[CP_UNROLL];
    uint32_t meta[CP_UNROLL], seg[CP_UNROLL];                   // meta: kind (0 nothing, 1 windows, 2 bytes) | shift of A << 4 | bytes of A << 9 | place of B << 14 (0: none)
#pragma unroll
    for (uint32_t u = 0; u < CP_UNROLL; ++u) {
        const int32_t o = 16 * (int32_t)(u * CP_THREADS + tid);
        meta[u] = 0; seg[u] = 0; va[u] = make_uint4(0, 0, 0, 0); vb[u] = make_uint4(0, 0, 0, 0);
        if (o + 16 <= rel_lo || o >= rel_hi || nseg == 0) continue;
        const int32_t x = o < rel_lo ? rel_lo : o;
        const int32_t vend = o + 16 < rel_hi ? o + 16 : rel_hi;
        uint32_t s = 0;                                         // the last unit that begins at x or in front of it
        for (uint32_t st = top; st; st >>= 1) s += (s + st < nseg && s_rel[s + st] <= x) ? st : 0;
        seg[u] = s;
        const int32_t b = s_rel[s], e = s_rel[s + 1];
        const int32_t dhi = vend < e ? vend : e;
        uint32_t kind = 1, sh = 0, place = 0;
        int64_t w = 0;
        if (e - b < 16) kind = 2;
        else {
            const int64_t delta = (int64_t)s_delta[s], qs = delta + x, wmax = delta + e - 16;
            w = qs < wmax ? qs : wmax;
            sh = (uint32_t)(qs - w);
        }
        if (dhi < vend) {                                       // the vector goes on into unit s + 1
            if (s + 1 >= nseg) kind = 2;
            else {
                const int32_t e2 = s_rel[s + 2];
                if (e2 < vend || e2 - e < 16) kind = 2; else place = (uint32_t)(e - o);      // 1 .. 15
            }
        }
        meta[u] = kind | (sh << 4) | ((uint32_t)(dhi - x) << 9) | (place << 14);
        if (kind == 1) {
            __builtin_memcpy(&va[u], at + w, 16);
            if (place) __builtin_memcpy(&vb[u], at + ((int64_t)s_delta[s + 1] + e), 16);
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < CP_UNROLL; ++u) {
        const int32_t o = 16 * (int32_t)(u * CP_THREADS + tid);
        const uint32_t kind = meta[u] & 3u;
        if (kind == 0) continue;
        const uint32_t klo = o < rel_lo ? (uint32_t)(rel_lo - o) : 0u;
        const uint32_t khi = o + 16 > rel_hi ? (uint32_t)(rel_hi - o) : 16u;
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
            int32_t e = s_rel[s + 1];
            int64_t delta = (int64_t)s_delta[s];
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                if (k < klo || k >= khi) continue;
                const int32_t d = o + (int32_t)k;
                while (d >= e && s + 1 < nseg) { ++s; e = s_rel[s + 1]; delta = (int64_t)s_delta[s]; }
                w[k >> 2] |= (uint32_t)at[delta + d] << (8 * (k & 3u));
            }
            r = make_uint4(w[0], w[1], w[2], w[3]);
        }
        uint8_t* po = out + t0 + o;
        if (klo == 0 && khi == 16) *(uint4*)po = r;
        else {
            const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k)
                if (k >= klo && k < khi) po[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3u)));
        }
    }
}

int fl_check_params(const char* who, const uq_filter_params* p, uint64_t nreads, uint64_t read_index_base) {
    UQ_REQUIRE(p, "%s: null argument", who);
    UQ_REQUIRE(p->unit == 1 || p->unit == 2, "%s: unit is %u, not 1 or 2", who, p->unit);
    UQ_REQUIRE(p->unit == 1 || ((nreads | read_index_base) & 1) == 0, "%s: unit 2 takes whole pairs: nreads %llu, read_index_base %llu", who,
               (unsigned long long)nreads, (unsigned long long)read_index_base);
    UQ_REQUIRE(p->min_len <= p->max_len, "%s: min_len %u > max_len %u", who, p->min_len, p->max_len);
    UQ_REQUIRE(p->min_mean_q <= 93, "%s: min_mean_q %u > 93", who, p->min_mean_q);
    return 0;
}
}  // namespace

extern "C" int uq_filter_report_init(uq_ctx* ctx, uq_filter_report* d_report) {
    UQ_REQUIRE(ctx && d_report, "uq_filter_report_init: null argument");
    UQ_CHECK_HIP(hipMemsetAsync(d_report, 0, sizeof(uq_filter_report), ctx->stream));
    return 0;
}

extern "C" int uq_filter_report_init_host(uq_filter_report* h_report) {
    UQ_REQUIRE(h_report, "uq_filter_report_init_host: null argument");
    memset(h_report, 0, sizeof(uq_filter_report));
    return 0;
}

extern "C" int uq_filter_mark(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                              uint64_t read_index_base, const uq_filter_params* h_params, uint8_t* d_verdict, uq_filter_report* d_report) {
    UQ_REQUIRE(ctx && d_line_start && d_report, "uq_filter_mark: null argument");
    UQ_TRY(fl_check_params("uq_filter_mark", h_params, nreads, read_index_base));
    UQ_REQUIRE(((uintptr_t)d_report & 7) == 0, "uq_filter_mark: d_report must be 8-byte aligned");
    if (nreads == 0) return 0;
    UQ_REQUIRE(d_buf && d_verdict, "uq_filter_mark: null argument");
    UQ_REQUIRE(first_read + nreads >= first_read && first_read + nreads < (1ull << 59), "uq_filter_mark: records beyond any index");
    // an upper bound of the tile count (a tile holds >= 1 record); surplus workgroups leave at once
    const uint32_t blocks = (uint32_t)(nreads < UQ_NUM_CU * 4 ? nreads : UQ_NUM_CU * 4);
    // the quality clamp: SWAR unless UQ_FILTER_CLAMP=lds asks for the 256-byte LDS table (tuning and tests; the verdicts are the same either way)
    const char* clamp = getenv("UQ_FILTER_CLAMP");
    if (clamp && strcmp(clamp, "lds") == 0)
        filter_mark_kernel<true><<<blocks, FM_THREADS, 0, ctx->stream>>>(d_buf, d_line_start, first_read, nreads, read_index_base, *h_params, d_verdict,
                                                                         (unsigned long long*)d_report);
    else
        filter_mark_kernel<false><<<blocks, FM_THREADS, 0, ctx->stream>>>(d_buf, d_line_start, first_read, nreads, read_index_base, *h_params, d_verdict,
                                                                          (unsigned long long*)d_report);
    UQ_LAUNCH_CHECK();
    return 0;
}

extern "C" int uq_filter_mark_host(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                                   uint64_t read_index_base, const uq_filter_params* h_params, uint8_t* h_verdict, uq_filter_report* h_report) {
    UQ_REQUIRE(h_line_start && h_report, "uq_filter_mark_host: null argument");
    UQ_TRY(fl_check_params("uq_filter_mark_host", h_params, nreads, read_index_base));
    if (nreads == 0) return 0;
    UQ_REQUIRE(h_buf && h_verdict, "uq_filter_mark_host: null argument");
    for (uint64_t i = 0; i < nreads; ++i) {
        const uint64_t* p = h_line_start + 4 * (first_read + i);
        UQ_REQUIRE(p[1] > p[0] && p[2] > p[1] && p[3] > p[2] && p[4] > p[3], "uq_filter_mark_host: record %llu: line starts out of order",
                   (unsigned long long)(first_read + i));
        const uint64_t Ls = p[2] - p[1] - 1, Lu = p[4] - p[3] - 1;
        uint64_t ncount = 0, qsum = 0;
        for (uint64_t k = 0; k < Ls; ++k) ncount += (h_buf[p[1] + k] | 0x20u) == 'n';
        for (uint64_t k = 0; k < Lu; ++k) { const uint32_t c = h_buf[p[3] + k]; qsum += (c < 33u ? 33u : (c > 126u ? 126u : c)) - 33u; }
        const uint32_t v = fl_verdict(*h_params, read_index_base + i, Ls, Lu, ncount, qsum);
        h_verdict[i] = (uint8_t)v;
        h_report->reads_in += 1; h_report->bases_in += Ls; h_report->bytes_in += p[4] - p[0];
        h_report->fail_min_len += v & 1u; h_report->fail_max_len += (v >> 1) & 1u; h_report->fail_max_n += (v >> 2) & 1u;
        h_report->fail_mean_q += (v >> 3) & 1u; h_report->fail_sample += (v >> 4) & 1u;
    }
    return 0;
}

extern "C" int uq_filter_plan(uq_ctx* ctx, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads, uint32_t unit, const uint8_t* d_verdict,
                              uint64_t* d_src, uint64_t* d_dst, uq_filter_report* d_report, uint64_t* h_kept_units, uint64_t* h_out_bytes) {
    UQ_REQUIRE(ctx && d_line_start && d_dst && d_report && h_kept_units && h_out_bytes, "uq_filter_plan: null argument");
    UQ_REQUIRE(unit == 1 || unit == 2, "uq_filter_plan: unit is %u, not 1 or 2", unit);
    UQ_REQUIRE(nreads % unit == 0, "uq_filter_plan: unit 2 takes whole pairs: nreads %llu", (unsigned long long)nreads);
    UQ_REQUIRE(((uintptr_t)d_report & 7) == 0, "uq_filter_plan: d_report must be 8-byte aligned");
    *h_kept_units = 0; *h_out_bytes = 0;
    if (nreads == 0) {
        UQ_CHECK_HIP(hipMemsetAsync(d_dst, 0, 8, ctx->stream));
        return 0;
    }
    UQ_REQUIRE(d_verdict && d_src, "uq_filter_plan: null argument");
    UQ_REQUIRE(first_read + nreads >= first_read && first_read + nreads < (1ull << 59), "uq_filter_plan: records beyond any index");
    const uint64_t nunits = nreads / unit;
    ScratchPlan sp;
    const size_t o_keep = sp.add(nunits * 8), o_len = sp.add(nunits * 8), o_tot = sp.add(16);
    void* ws;
    UQ_TRY(uq_scratch(ctx, sp.off, &ws));
    uint64_t* keep = (uint64_t*)((uint8_t*)ws + o_keep);
    uint64_t* len = (uint64_t*)((uint8_t*)ws + o_len);
    uint64_t* tot = (uint64_t*)((uint8_t*)ws + o_tot);
    const uint64_t want = (nunits + 255) / 256;
    const uint32_t blocks = (uint32_t)(want < UQ_NUM_CU * FP_BLOCKS_PER_CU ? want : UQ_NUM_CU * FP_BLOCKS_PER_CU);
    filter_units_kernel<<<blocks, 256, 0, ctx->stream>>>(d_line_start, first_read, nunits, unit, d_verdict, keep, len, (unsigned long long*)d_report);
    UQ_LAUNCH_CHECK();
    UQ_TRY(uq_scan_exclusive_u64(ctx, keep, keep, nunits, tot));
    UQ_TRY(uq_scan_exclusive_u64(ctx, len, len, nunits, tot + 1));
    filter_scatter_kernel<<<blocks, 256, 0, ctx->stream>>>(d_line_start, first_read, nunits, unit, keep, len, tot, d_src, d_dst, (unsigned long long*)d_report);
    UQ_LAUNCH_CHECK();
    UQ_TRY(uq_read_back(ctx, ctx->h_pinned, tot, 16));
    UQ_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    *h_kept_units = ctx->h_pinned[0]; *h_out_bytes = ctx->h_pinned[1];
    return 0;
}

extern "C" int uq_filter_plan_host(const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads, uint32_t unit, const uint8_t* h_verdict,
                                   uint64_t* h_src, uint64_t* h_dst, uq_filter_report* h_report, uint64_t* h_kept_units, uint64_t* h_out_bytes) {
    UQ_REQUIRE(h_line_start && h_dst && h_report && h_kept_units && h_out_bytes, "uq_filter_plan_host: null argument");
    UQ_REQUIRE(unit == 1 || unit == 2, "uq_filter_plan_host: unit is %u, not 1 or 2", unit);
    UQ_REQUIRE(nreads % unit == 0, "uq_filter_plan_host: unit 2 takes whole pairs: nreads %llu", (unsigned long long)nreads);
    UQ_REQUIRE(nreads == 0 || (h_verdict && h_src), "uq_filter_plan_host: null argument");
    uint64_t kept = 0, at = 0;
    for (uint64_t w = 0; w < nreads / unit; ++w) {
        const uint64_t* p = h_line_start + 4 * (first_read + w * unit);
        bool k = true;
        for (uint32_t m = 0; m < unit; ++m) k = k && h_verdict[w * unit + m] == 0;
        if (!k) {
            for (uint32_t m = 0; m < unit; ++m) h_report->fail_mate += h_verdict[w * unit + m] == 0;
            continue;
        }
        UQ_REQUIRE(p[4 * unit] >= p[0], "uq_filter_plan_host: record %llu: record starts out of order", (unsigned long long)(first_read + w * unit));
        h_src[kept] = p[0]; h_dst[kept] = at;
        at += p[4 * unit] - p[0]; ++kept;
        for (uint32_t m = 0; m < unit; ++m) h_report->bases_out += p[4 * m + 2] - p[4 * m + 1] - 1;
    }
    h_dst[kept] = at;
    h_report->reads_out += kept * unit; h_report->bytes_out += at;
    *h_kept_units = kept; *h_out_bytes = at;
    return 0;
}

extern "C" int uq_compact_records(uq_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes, const uint64_t* d_src, const uint64_t* d_dst, uint64_t kept_units,
                                  uint8_t* d_out, uint64_t out_capacity) {
    UQ_REQUIRE(ctx, "uq_compact_records: null argument");
    if (kept_units == 0) return 0;
    UQ_REQUIRE(d_buf && d_src && d_dst, "uq_compact_records: null argument");
    UQ_REQUIRE(kept_units < (1ull << 59), "uq_compact_records: units beyond any index");
    // the output's size, and the ends of the plan: nothing is launched on the buffers before the capacity has been checked
    uint64_t* h = ctx->h_pinned;
    void* ends;
    UQ_TRY(uq_scratch(ctx, 32, &ends));
    compact_ends_kernel<<<1, 1, 0, ctx->stream>>>(d_src, d_dst, kept_units, (uint64_t*)ends);
    UQ_LAUNCH_CHECK();
    UQ_TRY(uq_read_back(ctx, h, ends, 32));
    UQ_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    const uint64_t size = h[1];
    UQ_REQUIRE(h[0] == 0 && size >= 4 * kept_units && h[2] <= size, "uq_compact_records: the plan's offsets are out of order");
    UQ_REQUIRE(h[3] <= nbytes && size - h[2] <= nbytes - h[3], "uq_compact_records: the plan's last unit ends beyond the %llu bytes of the source",
               (unsigned long long)nbytes);
    UQ_REQUIRE(out_capacity >= size, "uq_compact_records: the output needs %llu bytes, out_capacity is %llu", (unsigned long long)size,
               (unsigned long long)out_capacity);
    UQ_REQUIRE(d_out, "uq_compact_records: null argument");
    const uint32_t mis = (uint32_t)((uintptr_t)d_out & 15u);
    const uint64_t ntiles = (size + mis + CP_TILE - 1) / CP_TILE;
    UQ_REQUIRE(ntiles < (1ull << 31), "uq_compact_records: more than 2^31 output tiles");
    void* ws;
    UQ_TRY(uq_scratch(ctx, (ntiles + 1) * 8, &ws));
    compact_origin_kernel<<<(uint32_t)((ntiles + 1 + 255) / 256), 256, 0, ctx->stream>>>(d_dst, kept_units, size, mis, ntiles, (uint64_t*)ws);
    UQ_LAUNCH_CHECK();
    compact_kernel<<<(uint32_t)ntiles, CP_THREADS, 0, ctx->stream>>>(d_buf, d_src, d_dst, kept_units, size, d_out, (const uint64_t*)ws);
    UQ_LAUNCH_CHECK();
    return 0;
}

extern "C" int uq_compact_records_host(const uint8_t* h_buf, uint64_t nbytes, const uint64_t* h_src, const uint64_t* h_dst, uint64_t kept_units,
                                       uint8_t* h_out, uint64_t out_capacity) {
    if (kept_units == 0) return 0;
    UQ_REQUIRE(h_buf && h_src && h_dst, "uq_compact_records_host: null argument");
    UQ_REQUIRE(out_capacity >= h_dst[kept_units], "uq_compact_records_host: the output needs %llu bytes, out_capacity is %llu",
               (unsigned long long)h_dst[kept_units], (unsigned long long)out_capacity);
    UQ_REQUIRE(h_out, "uq_compact_records_host: null argument");
    for (uint64_t j = 0; j < kept_units; ++j) {
        UQ_REQUIRE(h_dst[j + 1] >= h_dst[j] && h_src[j] <= nbytes && h_dst[j + 1] - h_dst[j] <= nbytes - h_src[j],
                   "uq_compact_records_host: unit %llu lies outside the source", (unsigned long long)j);
        memcpy(h_out + h_dst[j], h_buf + h_src[j], h_dst[j + 1] - h_dst[j]);
    }
    return 0;
}
