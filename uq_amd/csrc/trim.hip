// trim.hip -- read trimming (`--trim`).  An extension: the reference stores every read as it is given.
//
// uq_trim_mark gives every record its window [a, b) (the definition is in include/uqhip.h).  trim_mark_kernel is built like
// filter_mark_kernel (filter.hip; the stager is a copy, not shared): persistent workgroups walk tiles of R consecutive records, a tile is one
// contiguous span copied to LDS with coalesced 16-byte loads (the next tile's bytes are in flight, its bounds were asked for a turn earlier),
// P lanes (a power of two, 4 .. 16) share a record and take 8 bytes of a line per step.  The four steps of the definition depend on one
// another through [a, b), so a record is walked by ONE routine (tm_record) that a group of lanes runs together; what differs between the
// paths is where a line's bytes come from (LDS stage or HBM) and how the group reduces (shuffles inside a wave, or the whole workgroup
// through LDS):
//   poly-G and the N ends are reductions: the last position whose class is not G, the first and last whose class is not N -- a zero-byte test
//   on (w | 0x20) ^ 'g' over 8 bytes, walked from the window's end (or start) and left at the first step that finds one;
//   the quality sums are scans with an early stop: a lane sums its 8 terms T - q, an exclusive scan over the group's lanes gives each its
//   carry, the lane then finds its first negative prefix and its highest positive one, the group reduces (lowest stop, highest prefix, lowest
//   place among equals), the carry runs across a record's steps, and a record whose stop is found is walked no further.
// A tile beyond the stage is read straight from HBM: its records take a half-wave each, except those with a line beyond TM_LONG bytes, which
// the WHOLE workgroup walks (64-bit sums) -- never one thread along a line.  The report is kept as per-lane sums: one atomic per field per
// workgroup at the end.
//
// uq_trim_plan: trim_len_kernel writes every record's output length, uq_scan_exclusive_u64 turns them into offsets in place.
//
// uq_trim_records is built from the destination like compact_kernel (filter.hip): output tiles of TC_TILE bytes at 16-byte aligned ADDRESSES,
// trim_origin_kernel in front finds each tile's first record (a binary search over dst), the workgroup loads dst of its records (int32
// relative to the tile, saturated) and -- when the tile holds at most TC_NE records -- one 32-byte entry per record into LDS; an output byte of a
// record comes from one of five affine pieces of its source (qn '\n' | s[a:b] | '\n' p '\n' | u[a:b] | '\n'); pieces that are neighbours in
// the source as well are taken as one run, an item is one aligned output vector put together from at most three clamped 16-byte windows,
// one per run, or byte by byte where four or more runs meet.
#include "common.h"
#include "swar.h"

namespace {
enum { TR_READS_IN = 0, TR_BASES_IN, TR_BYTES_IN, TR_READS_TRIMMED, TR_BASES_OUT, TR_BYTES_OUT, TR_CUT_FIXED, TR_CUT_POLYG, TR_CUT_Q5, TR_CUT_Q3,
       TR_CUT_N, TR_EMPTIED, TR_LEN_MISMATCH, TR_WORDS };
static_assert(sizeof(uq_trim_report) == TR_WORDS * 8, "the report is thirteen u64 words");
static_assert(sizeof(uq_trim_params) == 32, "eight u32 words");

// a record's window and what each step cut (fixed, poly-G, q5, q3, N)
struct TmOut { uint32_t a, b; uint32_t cut[5]; };

// ---- the windows
constexpr int TM_THREADS = 256;
constexpr int TM_NV = 5;                          // 16-byte loads per lane per tile
constexpr uint32_t TM_CAP = TM_NV * 256 * 16;     // staging bytes per tile (20 KiB)
constexpr uint32_t TM_PAD = 16;                   // bytes in front of the stage: a window may begin up to 7 bytes in front of a line
constexpr uint32_t TM_RMAX = 64;                  // records per tile, upper bound (4 * TM_RMAX + 1 <= 2 * TM_THREADS)
constexpr uint64_t TM_LONG = 4096;                // in a tile beyond the stage: a line longer than this is walked by the whole workgroup, the others by a half-wave
constexpr uint64_t TM_H = 0x8080808080808080ull;
constexpr uint64_t TM_PAT_G = 0x6767676767676767ull, TM_PAT_N = 0x6E6E6E6E6E6E6E6Eull;
constexpr uint64_t TM_NONE = ~0ull;

// high bit of every byte of w that equals the byte of `pat` when its 0x20 bit is set (a letter of either case); exact, no carries between bytes
__device__ __forceinline__ uint64_t tm_eq_bits(uint64_t w, uint64_t pat) {
    const uint64_t x = (w | 0x2020202020202020ull) ^ pat;
    return ~(((x & ~TM_H) + ~TM_H) | x | ~TM_H);
}
// the high bits of the bytes j < n of an 8-byte window
__device__ __forceinline__ uint64_t tm_hb(uint32_t n) { return n >= 8 ? TM_H : (TM_H & ((1ull << (8 * n)) - 1)); }
__device__ __forceinline__ int32_t tm_q(uint32_t byte) { return (int32_t)(byte < 33u ? 33u : (byte > 126u ? 126u : byte)) - 33; }

// where a line's bytes come from: get8(pos) = the bytes pos .. pos + 7 of the line (pos >= -7; bytes outside the line are anything)
struct TmLdsLine {
    const uint8_t* stage; int32_t off;
    __device__ __forceinline__ uint64_t get8(int64_t pos) const {
        uint32_t lo, hi;
        lds_window8(stage, off + (int32_t)pos, lo, hi);
        return (uint64_t)lo | ((uint64_t)hi << 32);
    }
};
struct TmHbmLine {
    const uint8_t* p; uint64_t L;
    __device__ __forceinline__ uint64_t get8(int64_t pos) const {
        uint64_t w = 0;
        if (pos >= 0 && (uint64_t)pos + 8 <= L) __builtin_memcpy(&w, p + pos, 8);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const int64_t q = pos + j; if (q >= 0 && (uint64_t)q < L) w |= (uint64_t)p[q] << (8 * j); }
        }
        return w;
    }
};

// who walks a record together; every lane of a group runs the same trips.  K holds a position in a line the group walks.
// nl lanes of one wave (a power of two up to 32, aligned), for lines of at most 2^22 bytes: ballots and 32-bit shuffles.
struct TmLanes {
    typedef uint32_t K;
    uint32_t l, nl;
    __device__ __forceinline__ uint64_t mine(bool p) const { return (__ballot(p) >> (lane_id() & ~(nl - 1))) & ((1ull << nl) - 1); }
    template <typename T> __device__ __forceinline__ T excl(T v, T& total) const {
        T inc = v;
        for (uint32_t d = 1; d < nl; d <<= 1) { const T o = __shfl_up(inc, d, 64); if (l >= d) inc += o; }
        total = __shfl(inc, (int)(lane_id() | (nl - 1)), 64);
        return inc - v;
    }
    // `found` is TM_NONE or a position that grows with the lane: that of the first lane that has one
    __device__ __forceinline__ K first(K found) const {
        const uint64_t m = mine(found != (K)TM_NONE);
        const K v = __shfl(found, (int)((lane_id() & ~(nl - 1)) + (m ? (uint32_t)__ffsll((long long)m) - 1u : 0u)), 64);
        return m ? v : (K)TM_NONE;
    }
    // the first lane with `has`, nl if there is none
    __device__ __forceinline__ uint32_t first_lane(bool has) const {
        const uint64_t m = mine(has);
        return m ? (uint32_t)__ffsll((long long)m) - 1u : nl;
    }
    // over the lanes with `has`: the highest v (0 < v < 2^23) and the lowest krel (< 256) among equals, as one packed key
    template <typename T> __device__ __forceinline__ bool best(bool has, T v, uint32_t krel, T& bv, uint32_t& bk) const {
        uint32_t key = has ? ((uint32_t)v << 8) | (255u - krel) : 0u;
        for (uint32_t d = 1; d < nl; d <<= 1) { const uint32_t o = __shfl_xor(key, d, 64); key = o > key ? o : key; }
        bv = (T)(key >> 8); bk = 255u - (key & 255u);
        return key != 0;
    }
};
// the whole workgroup, through `red` (TM_THREADS / 64 + 1 words of LDS); every thread of the block makes every call
struct TmBlock {
    typedef uint64_t K;
    uint32_t l, nl; uint64_t* red;
    template <typename T> __device__ __forceinline__ T excl(T v, T& total) const { return block_exclusive_sum<T, TM_THREADS / 64>(v, (T*)red, total); }
    template <typename T> __device__ __forceinline__ T min(T v) const {
        v = wave_min(v);
        T* r = (T*)red;
        if (lane_id() == 0) r[threadIdx.x >> 6] = v;
        __syncthreads();
        T m = r[0];
        for (int w = 1; w < TM_THREADS / 64; ++w) m = r[w] < m ? r[w] : m;
        __syncthreads();
        return m;
    }
    template <typename T> __device__ __forceinline__ T max(T v) const {
        v = wave_max(v);
        T* r = (T*)red;
        if (lane_id() == 0) r[threadIdx.x >> 6] = v;
        __syncthreads();
        T m = r[0];
        for (int w = 1; w < TM_THREADS / 64; ++w) m = r[w] > m ? r[w] : m;
        __syncthreads();
        return m;
    }
    __device__ __forceinline__ K first(K found) const { return min(found); }
    __device__ __forceinline__ uint32_t first_lane(bool has) const { return min(has ? (uint32_t)threadIdx.x : (uint32_t)TM_THREADS); }
    template <typename T> __device__ __forceinline__ bool best(bool has, T v, uint32_t krel, T& bv, uint32_t& bk) const {
        bv = max(has ? v : (T)0);
        bk = min((has && v == bv) ? krel : 0xFFFFFFFFu);
        return bv > 0;
    }
};

// the number of consecutive bytes of class `pat` at the end of line[a, b): walked from b down, left at the first step that finds another byte
template <class G, class F>
__device__ __forceinline__ uint32_t tm_trailing_run(const G& g, const F& f, uint64_t pat, uint32_t a, uint32_t b) {
    typedef typename G::K K;
    const K n = b - a;
    for (K base = 0; base < n; base += 8 * g.nl) {
        const K k0 = base + 8 * g.l;
        K found = (K)TM_NONE;
        if (k0 < n) {
            const int64_t pos = (int64_t)b - (int64_t)k0 - 8;
            const uint32_t jlo = pos < (int64_t)a ? (uint32_t)((int64_t)a - pos) : 0u;
            const uint64_t m = ~tm_eq_bits(f.get8(pos), pat) & TM_H & ~tm_hb(jlo);
            if (m) found = k0 + (7u - ((63u - (uint32_t)__clzll((long long)m)) >> 3));
        }
        found = g.first(found);
        if (found != (K)TM_NONE) return (uint32_t)found;
    }
    return (uint32_t)n;
}
// ... at the start of line[a, b)
template <class G, class F>
__device__ __forceinline__ uint32_t tm_leading_run(const G& g, const F& f, uint64_t pat, uint32_t a, uint32_t b) {
    typedef typename G::K K;
    const K n = b - a;
    for (K base = 0; base < n; base += 8 * g.nl) {
        const K k0 = base + 8 * g.l;
        K found = (K)TM_NONE;
        if (k0 < n) {
            const uint32_t jhi = n - k0 < 8 ? (uint32_t)(n - k0) : 8u;
            const uint64_t m = ~tm_eq_bits(f.get8((int64_t)a + (int64_t)k0), pat) & tm_hb(jhi);
            if (m) found = k0 + (((uint32_t)__ffsll((long long)m) - 1u) >> 3);
        }
        found = g.first(found);
        if (found != (K)TM_NONE) return (uint32_t)found;
    }
    return (uint32_t)n;
}

// the bases the running sum cuts from one end of u[a, b): FWD from a up (5'), else from b - 1 down (3').  With x_k = T - q of the k-th byte in
// walking order and P_k their prefix sums: stop = the first k with P_k < 0; the answer is 1 + the first k in front of the stop with the highest
// P_k > 0, or 0.  Bytes beyond the window enter as x = 0: they neither stop nor raise the sum.  Acc holds 93 * (b - a).
template <typename Acc, bool FWD, class G, class F>
__device__ __forceinline__ uint32_t tm_qual_cut(const G& g, const F& f, uint32_t T, uint32_t a, uint32_t b) {
    typedef typename G::K K;
    const K n = b - a;
    Acc carry = 0, best = 0;
    K cut = 0;
    for (K base = 0; base < n; base += 8 * g.nl) {
        const K k0 = base + 8 * g.l;
        int32_t x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = 0;
        if (k0 < n) {
            const uint32_t cnt = n - k0 < 8 ? (uint32_t)(n - k0) : 8u;
            const uint64_t w = f.get8(FWD ? (int64_t)a + (int64_t)k0 : (int64_t)b - (int64_t)k0 - 8);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((uint32_t)j < cnt) x[j] = (int32_t)T - tm_q((uint32_t)(w >> (8 * (FWD ? j : 7 - j))) & 255u);
        }
        Acc sum = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += x[j];
        Acc total;
        Acc acc = carry + g.excl(sum, total);
        uint32_t lstop = 8, lbj = 8;
        Acc lb = best;
        if (k0 < n) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                acc += x[j];
                if (acc < 0 && lstop == 8) lstop = j;
                if (lstop == 8 && acc > lb) { lb = acc; lbj = j; }
            }
        }
        const uint32_t sl = g.first_lane(lstop < 8);                // the lane whose chunk holds the stop
        if (g.l > sl) lbj = 8;                                      // a chunk behind the stop
        Acc bv;
        uint32_t bk;
        if (g.best(lbj < 8, lb, 8 * g.l + lbj, bv, bk)) { best = bv; cut = base + bk + 1; }      // (a lane's lb is above `best`: the same test for every lane)
        if (sl < g.nl) break;                                       // the stop is found: the record is walked no further
        carry += total;
    }
    return (uint32_t)cut;
}

// step 1 of the definition (the one place it is written: kernel and host twin)
__host__ __device__ __forceinline__ void tm_fixed(const uq_trim_params& p, uint32_t L, uint32_t& a, uint32_t& b) {
    a = p.head < L ? p.head : L;
    b = L - (p.tail < L - a ? p.tail : L - a);
    if (p.crop != 0xFFFFFFFFu && (uint64_t)a + p.crop < b) b = a + p.crop;
}

// the window of a record whose two lines both hold L bytes, made by the lanes of g together; every lane gets the whole answer
template <typename Acc, class G, class F>
__device__ __forceinline__ TmOut tm_record(const G& g, const F& fs, const F& fu, uint32_t L, const uq_trim_params& p) {
    TmOut o;
    uint32_t a, b;
    tm_fixed(p, L, a, b);
    o.cut[0] = L - (b - a); o.cut[1] = o.cut[2] = o.cut[3] = o.cut[4] = 0;
    if (p.polyg && b > a) {
        const uint32_t run = tm_trailing_run(g, fs, TM_PAT_G, a, b);
        if (run >= p.polyg) { b -= run; o.cut[1] = run; }
    }
    if ((p.q3 | p.q5) && b > a) {
        const uint32_t c3 = p.q3 ? tm_qual_cut<Acc, false>(g, fu, p.q3, a, b) : 0u;
        const uint32_t c5 = p.q5 ? tm_qual_cut<Acc, true>(g, fu, p.q5, a, b) : 0u;
        const uint32_t b2 = b - c3, a2 = a + c5 < b2 ? a + c5 : b2;
        o.cut[3] = c3; o.cut[2] = a2 - a;
        a = a2; b = b2;
    }
    if ((p.flags & UQ_TRIM_N) && b > a) {
        const uint32_t lead = tm_leading_run(g, fs, TM_PAT_N, a, b);
        a += lead; o.cut[4] = lead;
        if (b > a) { const uint32_t tr = tm_trailing_run(g, fs, TM_PAT_N, a, b); b -= tr; o.cut[4] += tr; }
    }
    o.a = a; o.b = b;
    return o;
}

struct TmAcc {
    uint64_t bases = 0, cut[5] = {0, 0, 0, 0, 0};
    uint32_t reads = 0, trimmed = 0, emptied = 0, mismatch = 0;      // < 2^32: a lane sees fewer than 2^32 records
    __device__ __forceinline__ void record(const TmOut& o, uint64_t Ls, bool mis) {
        ++reads; bases += Ls;
        if (mis) { ++mismatch; return; }
#pragma unroll
        for (int k = 0; k < 5; ++k) cut[k] += o.cut[k];
        trimmed += !(o.a == 0 && o.b == Ls);
        emptied += o.a == o.b && Ls > 0;
    }
};

__global__ __launch_bounds__(TM_THREADS) void trim_mark_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ ls, uint64_t first, uint64_t n,
                                                               uq_trim_params prm, uint32_t* __restrict__ window, unsigned long long* __restrict__ report) {
    __shared__ __align__(16) uint8_t stage_raw[TM_PAD + TM_CAP + 32];
    __shared__ uint32_t meta[4 * TM_RMAX + 4];
    __shared__ uint32_t cfg[2];
    __shared__ uint64_t red[TM_THREADS / 64][10];
    __shared__ uint64_t tot[10];
    uint8_t* const stage = stage_raw + TM_PAD;
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    // the tile geometry is decided here from the shard's average record length (no round trip in front of the launch, as in filter.hip)
    if (tid == 0) {
        const uint64_t avg = (ls[4 * (first + n)] - ls[4 * first]) / n + 1;
        uint64_t R = (TM_CAP - 64) / (avg + avg / 8 + 1);
        R = R > TM_RMAX ? TM_RMAX : (R < 1 ? 1 : R);
        uint32_t P = 16;
        while (P > 1 && P * (uint32_t)R > TM_THREADS) P >>= 1;      // a power of two: the lanes of a record reduce with shuffles
        cfg[0] = (uint32_t)R; cfg[1] = P;
    }
    __syncthreads();
    const uint32_t R = __builtin_amdgcn_readfirstlane(cfg[0]), P = __builtin_amdgcn_readfirstlane(cfg[1]);
    const uint64_t ntiles = (n + R - 1) / R;
    const uint32_t rr = tid / P, pp = tid & (P - 1);
    TmAcc acc;

    const uint64_t S = gridDim.x;
    struct Bounds { uint64_t g0, g1; };
    struct Regs { uint4 v[TM_NV]; uint64_t m0, m1; uint64_t g0; uint32_t skew, nvec, Rt; bool exists, staged; };
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
        for (int u = 0; u < TM_NV; ++u) x.v[u] = make_uint4(0, 0, 0, 0);
        if (!x.exists) return x;
        x.Rt = (uint32_t)((n - tt * R) < R ? (n - tt * R) : R);
        const uint64_t a0 = ((uint64_t)(uintptr_t)buf + b.g0) & ~uint64_t(15);
        x.skew = (uint32_t)(((uint64_t)(uintptr_t)buf + b.g0) - a0);
        const uint64_t span = b.g1 - b.g0 + x.skew;
        x.staged = span + 16 <= TM_CAP;
        if (!x.staged) return x;
        x.nvec = (uint32_t)((span + 15) >> 4);
        const uint4* src = (const uint4*)(buf + ((int64_t)b.g0 - (int64_t)x.skew));      // aligned vectors that hold at least one byte of the span
#pragma unroll
        for (int u = 0; u < TM_NV; ++u) { const uint32_t i = u * TM_THREADS + tid; if (i < x.nvec) x.v[u] = src[i]; }
        const uint64_t* lsp = ls + 4 * (first + tt * R);
        if (tid <= 4 * x.Rt) x.m0 = lsp[tid];
        if (tid + TM_THREADS <= 4 * x.Rt) x.m1 = lsp[tid + TM_THREADS];
        return x;
    };
    const TmOut unchanged_proto = {0, 0, {0, 0, 0, 0, 0}};

    uint64_t t = blockIdx.x;
    Bounds b_next = load_bounds(t + S);
    Regs cur = issue(t, load_bounds(t));
    for (; t < ntiles; t += S) {
        const uint64_t r0 = t * R;
        const uint32_t Rt = cur.Rt;
        const Bounds b_nn = load_bounds(t + 2 * S);
        if (cur.staged) {
            if (tid <= 4 * Rt) meta[tid] = (uint32_t)(cur.m0 - cur.g0) + cur.skew;
            if (tid + TM_THREADS <= 4 * Rt) meta[tid + TM_THREADS] = (uint32_t)(cur.m1 - cur.g0) + cur.skew;
#pragma unroll
            for (int u = 0; u < TM_NV; ++u) { const uint32_t i = u * TM_THREADS + tid; if (i < cur.nvec) ((uint4*)stage)[i] = cur.v[u]; }
        }
        __syncthreads();
        const bool staged = cur.staged;
        cur = issue(t + S, b_next);          // the next tile's loads fly while this one is trimmed
        b_next = b_nn;
        if (staged) {
            if (rr < Rt) {                   // (the same for the P lanes of a record: they shuffle among themselves only)
                const uint32_t s = meta[4 * rr + 1], e1 = meta[4 * rr + 2], q = meta[4 * rr + 3], e2 = meta[4 * rr + 4];
                const uint32_t Ls = e1 - s - 1, Lu = e2 - q - 1;
                TmOut o = unchanged_proto;
                o.b = Ls;
                if (Ls == Lu) {
                    const TmLanes g{pp, P};
                    const TmLdsLine fs{stage, (int32_t)s}, fu{stage, (int32_t)q};
                    o = tm_record<int32_t>(g, fs, fu, Ls, prm);      // a staged line is shorter than the stage: the sums fit 32 bits
                }
                if (pp == 0) {
                    window[2 * (r0 + rr)] = o.a; window[2 * (r0 + rr) + 1] = o.b;
                    acc.record(o, Ls, Ls != Lu);
                }
            }
        } else {
            // a span beyond the stage (a long read in it, or a run of longer-than-average ones): straight from HBM.  Records whose lines
            // are at most TM_LONG bytes take a half-wave each, eight at a time, with no barrier; a record with longer lines is walked by
            // the whole workgroup.
            const uint64_t* lsp = ls + 4 * (first + r0);
            for (uint32_t rb = 2 * wave; rb < Rt; rb += 2 * (TM_THREADS / 64)) {
                const uint32_t r = rb + (lane >> 5), hl = lane & 31u;
                if (r < Rt) {                // (the same for the 32 lanes of a half-wave)
                    const uint64_t* p = lsp + 4 * r;
                    const uint64_t s = p[1], e1 = p[2], q = p[3], e2 = p[4];
                    const uint64_t Ls = e1 - s - 1, Lu = e2 - q - 1;
                    if (Ls != Lu || Ls <= TM_LONG) {
                        TmOut o = unchanged_proto;
                        o.b = (uint32_t)Ls;
                        if (Ls == Lu) {
                            const TmLanes g{hl, 32u};
                            const TmHbmLine fs{buf + s, Ls}, fu{buf + q, Lu};
                            o = tm_record<int32_t>(g, fs, fu, (uint32_t)Ls, prm);
                        }
                        if (hl == 0) {
                            window[2 * (r0 + r)] = o.a; window[2 * (r0 + r) + 1] = o.b;
                            acc.record(o, Ls, Ls != Lu);
                        }
                    }
                }
            }
            for (uint32_t r = 0; r < Rt; ++r) {
                const uint64_t* p = lsp + 4 * r;
                const uint64_t s = p[1], e1 = p[2], q = p[3], e2 = p[4];
                const uint64_t Ls = e1 - s - 1, Lu = e2 - q - 1;
                if (Ls != Lu || Ls <= TM_LONG) continue;                               // (the same for every thread: no barrier is skipped by some)
                const TmBlock g{tid, (uint32_t)TM_THREADS, &red[0][0]};
                const TmHbmLine fs{buf + s, Ls}, fu{buf + q, Lu};
                const TmOut o = tm_record<int64_t>(g, fs, fu, (uint32_t)Ls, prm);
                if (tid == 0) {
                    window[2 * (r0 + r)] = o.a; window[2 * (r0 + r) + 1] = o.b;
                    acc.record(o, Ls, false);
                }
            }
        }
        __syncthreads();
    }
    // the report: per-lane sums -> one atomic per field per workgroup.  bases_out and bytes_out follow from what was cut: a record loses two
    // bytes per base; the one thread that adds bytes_in adds it to bytes_out too, every workgroup takes its cuts off (modulo 2^64).
    uint64_t f[10] = {acc.reads, acc.bases, acc.trimmed, acc.cut[0], acc.cut[1], acc.cut[2], acc.cut[3], acc.cut[4], acc.emptied, acc.mismatch};
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 10; ++k) { f[k] = wave_sum(f[k]); if (lane == 0) red[wave][k] = f[k]; }
    __syncthreads();
    if (tid < 10) {
        uint64_t v = 0;
        for (int w = 0; w < TM_THREADS / 64; ++w) v += red[w][tid];
        tot[tid] = v;
        const uint32_t field = tid == 0 ? TR_READS_IN : (tid == 1 ? TR_BASES_IN : (tid == 2 ? TR_READS_TRIMMED : (tid < 8 ? TR_CUT_FIXED + (tid - 3) : TR_EMPTIED + (tid - 8))));
        if (v) atomicAdd(report + field, (unsigned long long)v);
    }
    __syncthreads();
    if (tid == 0) {
        const uint64_t cuts = tot[3] + tot[4] + tot[5] + tot[6] + tot[7];
        uint64_t bytes = 0 - 2 * cuts;
        if (blockIdx.x == 0) {
            const uint64_t all = ls[4 * (first + n)] - ls[4 * first];
            atomicAdd(report + TR_BYTES_IN, (unsigned long long)all);
            bytes += all;
        }
        if (tot[1] - cuts) atomicAdd(report + TR_BASES_OUT, (unsigned long long)(tot[1] - cuts));
        if (bytes) atomicAdd(report + TR_BYTES_OUT, (unsigned long long)bytes);
    }
}

// ---- the plan
constexpr uint32_t TP_BLOCKS_PER_CU = 8;

__global__ __launch_bounds__(256) void trim_len_kernel(const uint64_t* __restrict__ ls, uint64_t first, uint64_t n, const uint32_t* __restrict__ window,
                                                       uint64_t* __restrict__ len) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t* p = ls + 4 * (first + i);
        const uint64_t Ls = p[2] - p[1] - 1, Lu = p[4] - p[3] - 1;
        const uint64_t a = window[2 * i], b = window[2 * i + 1];
        len[i] = (p[4] - p[0]) - (Ls == Lu ? 2 * (Ls - (b - a)) : 0);
    }
}

// ---- the copy
constexpr int TC_THREADS = 256;
constexpr uint32_t TC_UNROLL = 4;                               // 16-byte vectors a lane has in flight
constexpr uint32_t TC_TILE = TC_THREADS * TC_UNROLL * 16;       // bytes of output per tile, 16 KiB (tests/test_gpu_trim.py builds its inputs from this)
constexpr uint32_t TC_NP = TC_TILE / 4 + 3;                     // record starts a tile can need: an output record is >= 4 bytes (four newlines), + the one that begins in front + the end
constexpr uint32_t TC_NE = TC_TILE / 16 + 3;                    // records whose entries are kept in LDS (records of 16 bytes and more on average); beyond: read from the index
constexpr uint32_t TC_BLOCKS_PER_CU = 3;                        // what 4 x TC_NP + 32 x TC_NE = 49 260 bytes of LDS admit
constexpr int64_t TC_FAR = 1 << 29;                             // where the relative starts saturate

// The copy works on UNITS: unit i is record i shifted one byte down -- the '\n' that ends record i - 1, then record i without its own last
// '\n' (unit 0 has no byte in front of it, the last unit keeps its '\n').  That '\n' and the QNAME line behind it are neighbours in the source
// as well, so a unit is four pieces (['\n'] qn '\n' | s[a:b] | '\n' p '\n' | u[a:b]) and no piece is a single byte.
struct __align__(16) TcEntry { uint64_t src; uint32_t A1, a, n, Ls, Lp, Lu; };      // where the unit's source begins; A1 = its first piece
static_assert(sizeof(TcEntry) == 32, "32-byte entries");

__device__ __forceinline__ uint64_t tc_ustart(const uint64_t* __restrict__ dst, uint64_t i, uint64_t n) { return dst[i] - (i > 0 && i < n ? 1u : 0u); }
__device__ __forceinline__ TcEntry tc_entry(const uint64_t* __restrict__ ls, const uint32_t* __restrict__ window, uint64_t first, uint64_t i) {
    const uint64_t* p = ls + 4 * (first + i);
    const uint64_t p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4];
    const uint32_t lead = i > 0 ? 1u : 0u;
    TcEntry e;
    e.src = p0 - lead; e.A1 = (uint32_t)(p1 - p0) + lead; e.Ls = (uint32_t)(p2 - p1 - 1); e.Lp = (uint32_t)(p3 - p2 - 1); e.Lu = (uint32_t)(p4 - p3 - 1);
    e.a = window[2 * i]; e.n = window[2 * i + 1] - e.a;
    return e;
}
// the source bytes of the unit: no window leaves them (the last unit: with its '\n')
__device__ __forceinline__ uint64_t tc_src_len(const TcEntry& e, bool last) { return (uint64_t)e.A1 + e.Ls + e.Lp + e.Lu + 2 + (last ? 1 : 0); }
// The output byte d of the unit is the source byte d + shift of the unit.  Pieces that follow one another in the source as well (a = 0: the
// QNAME and the sequence, the third line and the qualities; b = Ls: the sequence and the third line) make one RUN: it ends in front of `end`.
__device__ __forceinline__ void tc_run(const TcEntry& e, int64_t d, int64_t& shift, int64_t& end) {
    const int64_t n4 = e.Lu == e.Ls ? (int64_t)e.n : (int64_t)e.Lu;          // (lines of different lengths: the record as it is, a = 0 and n = Ls)
    const int64_t gap = (int64_t)e.Ls - e.n;
    int64_t c[5], sh[5];
    c[0] = e.A1; c[1] = c[0] + e.n; c[2] = c[1] + e.Lp + 2; c[3] = c[2] + n4; c[4] = c[3] + 1;
    sh[0] = 0; sh[1] = e.a; sh[2] = gap; sh[3] = gap + e.a; sh[4] = gap + (int64_t)e.Lu - n4;
    bool open = false, done = false;
    shift = sh[4]; end = c[4];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        if (!open) {
            if (d < c[j]) { open = true; shift = sh[j]; end = c[j]; }
        } else if (!done && j > 0 && c[j] != c[j > 0 ? j - 1 : 0]) {      // (an empty piece ends no run)
            if (sh[j] == shift) end = c[j]; else done = true;
        }
    }
}

__device__ __forceinline__ uint64_t tc_tile_lo(uint64_t t, uint32_t mis, uint64_t size) {
    if (t == 0) return 0;
    const uint64_t o = t * TC_TILE - mis;
    return o < size ? o : size;
}

// the words uq_trim_records checks before it launches anything on the buffers, gathered for one read-back
__global__ void trim_ends_kernel(const uint64_t* __restrict__ ls, uint64_t first, uint64_t n, const uint64_t* __restrict__ dst, uint64_t* __restrict__ out) {
    out[0] = dst[0]; out[1] = dst[n]; out[2] = dst[n - 1]; out[3] = ls[4 * (first + n)];
}

// origin[t] = the last unit i in [0, n) that begins at tc_tile_lo(t) or in front of it, for t in [0, ntiles]
__global__ __launch_bounds__(256) void trim_origin_kernel(const uint64_t* __restrict__ dst, uint64_t n, uint64_t size, uint32_t mis, uint64_t ntiles,
                                                          uint64_t* __restrict__ origin) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > ntiles) return;
    const uint64_t x = tc_tile_lo(t, mis, size);
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (tc_ustart(dst, mid, n) <= x) lo = mid; else hi = mid;
    }
    origin[t] = lo;
}

__global__ __launch_bounds__(TC_THREADS, TC_BLOCKS_PER_CU) void trim_copy_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ ls, uint64_t first,
                                                                                  uint64_t n, const uint32_t* __restrict__ window,
                                                                                  const uint64_t* __restrict__ dst, uint64_t size, uint8_t* __restrict__ out,
                                                                                  const uint64_t* __restrict__ origin) {
    __shared__ TcEntry s_ent[TC_NE];                            // unit U0 + j, when the tile holds at most TC_NE units
    __shared__ int32_t s_rel[TC_NP];                            // where unit U0 + j begins relative to the tile's first vector, saturated at +- TC_FAR
    const uint32_t tid = threadIdx.x;
    const uint64_t t = blockIdx.x;
    const uint32_t mis = (uint32_t)((uintptr_t)out & 15u);
    const int64_t t0 = (int64_t)(t * TC_TILE) - (int64_t)mis;   // output offset of the tile's first vector (negative in tile 0 of a misaligned buffer)
    const uint64_t U0 = origin[t];
    uint64_t last = origin[t + 1] + 1;                          // the entry behind the last unit that can begin inside the tile: it closes that unit
    if (last > n) last = n;
    const uint64_t cnt64 = last - U0 + 1;
    const uint32_t cnt = (uint32_t)(cnt64 < TC_NP ? cnt64 : TC_NP);
    const uint32_t nseg = cnt - 1;                              // unit j, j < nseg, covers the relative output offsets [rel(j), rel(j + 1))
    const bool in_lds = nseg <= TC_NE;
    for (uint32_t j = tid; j < cnt; j += TC_THREADS) {
        int64_t rel = (int64_t)tc_ustart(dst, U0 + j, n) - t0;
        rel = rel < -TC_FAR ? -TC_FAR : (rel > TC_FAR ? TC_FAR : rel);
        s_rel[j] = (int32_t)rel;
        if (in_lds && j < nseg) s_ent[j] = tc_entry(ls, window, first, U0 + j);
    }
    const int64_t rel0 = (int64_t)tc_ustart(dst, U0, n) - t0;   // exact: only the tile's first unit can begin far in front of it
    __syncthreads();
    const uint32_t top = nseg > 1 ? 1u << (31 - __clz((int)(nseg - 1))) : 0u;
    // the output's bounds relative to the tile
    const int32_t rel_lo = t0 < 0 ? (int32_t)(-t0) : 0;
    const int64_t left = (int64_t)size - t0;
    const int32_t rel_hi = left < (int64_t)TC_TILE ? (int32_t)left : (int32_t)TC_TILE;
    auto entry_of = [&](uint32_t j) -> TcEntry { return in_lds ? s_ent[j] : tc_entry(ls, window, first, U0 + j); };
    auto rel_of = [&](uint32_t j) -> int64_t { return j == 0 ? rel0 : (int64_t)s_rel[j]; };

    // A window is 16 source bytes that hold the bytes of one run a vector needs: at the run's byte, or ending with the unit's source and
    // shifted down.  No window leaves its unit.  A vector takes up to three; where four or more runs meet, or a unit's source is under 16
    // bytes, it goes byte by byte.
    typedef unsigned __int128 u128;
    uint4 vw[TC_UNROLL][3];
    uint32_t m0[TC_UNROLL], m1[TC_UNROLL], seg[TC_UNROLL];      // m0: kind (0 nothing, 1 windows, 2 bytes) | window 0 << 2 | window 1 << 16; m1: window 2
                                                                // a window: has | shift << 1 | bytes << 5 | place << 10 (14 bits)
#pragma unroll
    for (uint32_t u = 0; u < TC_UNROLL; ++u) {
        const int32_t o = 16 * (int32_t)(u * TC_THREADS + tid);
        m0[u] = 0; m1[u] = 0; seg[u] = 0;
#pragma unroll
        for (int w = 0; w < 3; ++w) vw[u][w] = make_uint4(0, 0, 0, 0);
        if (o + 16 <= rel_lo || o >= rel_hi || nseg == 0) continue;
        const int32_t x = o < rel_lo ? rel_lo : o;
        const int32_t vend = o + 16 < rel_hi ? o + 16 : rel_hi;
        uint32_t s = 0;                                         // the last unit that begins at x or in front of it
        for (uint32_t st = top; st; st >>= 1) s += (s + st < nseg && s_rel[s + st] <= x) ? st : 0;
        seg[u] = s;
        TcEntry E = entry_of(s);
        int64_t rs = rel_of(s), e = s_rel[s + 1];
        uint32_t kind = 1, mw[3] = {0, 0, 0};
        int64_t wa[3] = {0, 0, 0};
        int32_t pos = x;
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            if (kind != 1 || pos >= vend) continue;
            if (pos >= e) {                                     // on into the next unit
                ++s;
                if (s >= nseg) { kind = 2; continue; }
                E = entry_of(s); rs = rel_of(s); e = s_rel[s + 1];
            }
            const uint64_t len = tc_src_len(E, U0 + s + 1 == n);
            if (len < 16) { kind = 2; continue; }
            int64_t shift, end;
            tc_run(E, (int64_t)pos - rs, shift, end);
            int64_t pe = rs + end;
            pe = pe < e ? pe : e;
            const int32_t stop = pe < vend ? (int32_t)pe : vend;
            const int64_t so = (int64_t)pos - rs + shift, wmax = (int64_t)len - 16;
            const int64_t wv = so < wmax ? so : wmax;
            wa[w] = (int64_t)E.src + wv;
            mw[w] = 1u | ((uint32_t)(so - wv) << 1) | ((uint32_t)(stop - pos) << 5) | ((uint32_t)(pos - o) << 10);
            pos = stop;
        }
        if (pos < vend) kind = 2;
        m0[u] = kind | (kind == 1 ? (mw[0] << 2) | (mw[1] << 16) : 0u);
        m1[u] = kind == 1 ? mw[2] : 0u;
        if (kind == 1) {
#pragma unroll
            for (int w = 0; w < 3; ++w)
                if (mw[w]) __builtin_memcpy(&vw[u][w], buf + wa[w], 16);
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < TC_UNROLL; ++u) {
        const int32_t o = 16 * (int32_t)(u * TC_THREADS + tid);
        const uint32_t kind = m0[u] & 3u;
        if (kind == 0) continue;
        const uint32_t klo = o < rel_lo ? (uint32_t)(rel_lo - o) : 0u;
        const uint32_t khi = o + 16 > rel_hi ? (uint32_t)(rel_hi - o) : 16u;
        uint4 r;
        if (kind == 1) {
            const uint32_t mw[3] = {(m0[u] >> 2) & 0x3FFFu, (m0[u] >> 16) & 0x3FFFu, m1[u]};
            u128 R = 0;
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                if (!mw[w]) continue;
                u128 A;
                __builtin_memcpy(&A, &vw[u][w], 16);
                const uint32_t len = (mw[w] >> 5) & 31u;
                A >>= 8 * ((mw[w] >> 1) & 15u);
                if (len < 16) A &= ((u128)1 << (8 * len)) - 1;
                R |= A << (8 * ((mw[w] >> 10) & 15u));
            }
            __builtin_memcpy(&r, &R, 16);
        } else {
            uint32_t s = seg[u];
            TcEntry E = entry_of(s);
            int64_t rs = rel_of(s), e = s_rel[s + 1], shift = 0, pe = rs;       // (pe = rs: the first byte looks its run up)
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t k = klo; k < khi; ++k) {
                const int64_t d = o + (int32_t)k;
                if (d >= pe) {
                    while (d >= e && s + 1 < nseg) { ++s; E = entry_of(s); rs = rel_of(s); e = s_rel[s + 1]; }
                    int64_t end;
                    tc_run(E, d - rs, shift, end);
                    pe = rs + end;
                    pe = pe < e ? pe : e;
                }
                const uint32_t byte = buf[(int64_t)E.src + (d - rs) + shift];
                w[k >> 2] |= byte << (8 * (k & 3u));
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

// the record index of the trimmed text from dst, the old index and the windows
__global__ __launch_bounds__(256) void trim_index_kernel(const uint64_t* __restrict__ ls, uint64_t first, uint64_t n, const uint32_t* __restrict__ window,
                                                         const uint64_t* __restrict__ dst, uint64_t* __restrict__ lso) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t* p = ls + 4 * (first + i);
        const uint64_t d = dst[i], ns = (uint64_t)window[2 * i + 1] - window[2 * i];
        lso[4 * i] = d;
        lso[4 * i + 1] = d + (p[1] - p[0]);
        lso[4 * i + 2] = d + (p[1] - p[0]) + ns + 1;
        lso[4 * i + 3] = d + (p[1] - p[0]) + ns + 1 + (p[3] - p[2]);
        if (i + 1 == n) lso[4 * n] = dst[n];
    }
}

int tm_check_params(const char* who, const uq_trim_params* p) {
    UQ_REQUIRE(p, "%s: null argument", who);
    UQ_REQUIRE(p->q5 <= 93, "%s: q5 %u > 93", who, p->q5);
    UQ_REQUIRE(p->q3 <= 93, "%s: q3 %u > 93", who, p->q3);
    UQ_REQUIRE(p->crop != 0, "%s: crop is 0 (UINT32_MAX switches it off)", who);
    return 0;
}

// the 3' / 5' running sums of the definition, as they are written there
void tm_host_quality(const uint8_t* u, uint32_t a, uint32_t b, uint32_t T3, uint32_t T5, uint32_t& a2, uint32_t& b2) {
    a2 = a; b2 = b;
    if (T3) {
        int64_t acc = 0, best = 0;
        for (uint32_t i = b; i-- > a;) {
            const uint32_t c = u[i];
            acc += (int64_t)T3 - (int64_t)((c < 33u ? 33u : (c > 126u ? 126u : c)) - 33u);
            if (acc < 0) break;
            if (acc > best) { best = acc; b2 = i; }
        }
    }
    if (T5) {
        int64_t acc = 0, best = 0;
        for (uint32_t i = a; i < b; ++i) {
            const uint32_t c = u[i];
            acc += (int64_t)T5 - (int64_t)((c < 33u ? 33u : (c > 126u ? 126u : c)) - 33u);
            if (acc < 0) break;
            if (acc > best) { best = acc; a2 = i + 1; }
        }
    }
}

// a record's lines from the index, checked: the starts in order, the lines shorter than 2^32
int tm_host_lines(const char* who, const uint64_t* p, uint64_t r, uint64_t& Ls, uint64_t& Lu) {
    UQ_REQUIRE(p[1] > p[0] && p[2] > p[1] && p[3] > p[2] && p[4] > p[3], "%s: record %llu: line starts out of order", who, (unsigned long long)r);
    UQ_REQUIRE(p[1] - p[0] <= 0xFFFFFFFFull && p[2] - p[1] <= 0xFFFFFFFFull && p[3] - p[2] <= 0xFFFFFFFFull && p[4] - p[3] <= 0xFFFFFFFFull,
               "%s: record %llu: a line of 2^32 bytes or more", who, (unsigned long long)r);
    Ls = p[2] - p[1] - 1; Lu = p[4] - p[3] - 1;
    return 0;
}
// ... and its window: a <= b <= Ls, and (0, Ls) where the two lines differ in length
int tm_host_window(const char* who, uint64_t r, uint64_t Ls, uint64_t Lu, uint32_t a, uint32_t b) {
    UQ_REQUIRE(a <= b && b <= Ls, "%s: record %llu: the window (%u, %u) does not lie in a line of %llu bytes", who, (unsigned long long)r, a, b,
               (unsigned long long)Ls);
    UQ_REQUIRE(Ls == Lu || (a == 0 && b == Ls), "%s: record %llu: lines of %llu and %llu bytes are copied unchanged, the window is (%u, %u)", who,
               (unsigned long long)r, (unsigned long long)Ls, (unsigned long long)Lu, a, b);
    return 0;
}
}  // namespace

extern "C" int uq_trim_report_init(uq_ctx* ctx, uq_trim_report* d_report) {
    UQ_REQUIRE(ctx && d_report, "uq_trim_report_init: null argument");
    UQ_CHECK_HIP(hipMemsetAsync(d_report, 0, sizeof(uq_trim_report), ctx->stream));
    return 0;
}

extern "C" int uq_trim_report_init_host(uq_trim_report* h_report) {
    UQ_REQUIRE(h_report, "uq_trim_report_init_host: null argument");
    memset(h_report, 0, sizeof(uq_trim_report));
    return 0;
}

extern "C" int uq_trim_mark(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                            const uq_trim_params* h_params, uint32_t* d_window, uq_trim_report* d_report) {
    UQ_REQUIRE(ctx && d_line_start && d_report, "uq_trim_mark: null argument");
    UQ_TRY(tm_check_params("uq_trim_mark", h_params));
    UQ_REQUIRE(((uintptr_t)d_report & 7) == 0, "uq_trim_mark: d_report must be 8-byte aligned");
    if (nreads == 0) return 0;
    UQ_REQUIRE(d_buf && d_window, "uq_trim_mark: null argument");
    UQ_REQUIRE(((uintptr_t)d_window & 3) == 0, "uq_trim_mark: d_window must be 4-byte aligned");
    UQ_REQUIRE(first_read + nreads >= first_read && first_read + nreads < (1ull << 59), "uq_trim_mark: records beyond any index");
    // an upper bound of the tile count (a tile holds >= 1 record); surplus workgroups leave at once
    const uint32_t blocks = (uint32_t)(nreads < UQ_NUM_CU * 4 ? nreads : UQ_NUM_CU * 4);
    trim_mark_kernel<<<blocks, TM_THREADS, 0, ctx->stream>>>(d_buf, d_line_start, first_read, nreads, *h_params, d_window, (unsigned long long*)d_report);
    UQ_LAUNCH_CHECK();
    return 0;
}

extern "C" int uq_trim_mark_host(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                                 const uq_trim_params* h_params, uint32_t* h_window, uq_trim_report* h_report) {
    UQ_REQUIRE(h_line_start && h_report, "uq_trim_mark_host: null argument");
    UQ_TRY(tm_check_params("uq_trim_mark_host", h_params));
    if (nreads == 0) return 0;
    UQ_REQUIRE(h_buf && h_window, "uq_trim_mark_host: null argument");
    const uq_trim_params& prm = *h_params;
    for (uint64_t i = 0; i < nreads; ++i) {
        const uint64_t* p = h_line_start + 4 * (first_read + i);
        uint64_t Ls, Lu;
        UQ_TRY(tm_host_lines("uq_trim_mark_host", p, first_read + i, Ls, Lu));
        const uint8_t* s = h_buf + p[1];
        const uint8_t* u = h_buf + p[3];
        h_report->reads_in += 1; h_report->bases_in += Ls; h_report->bytes_in += p[4] - p[0];
        if (Ls != Lu) {
            h_window[2 * i] = 0; h_window[2 * i + 1] = (uint32_t)Ls;
            h_report->len_mismatch += 1; h_report->bases_out += Ls; h_report->bytes_out += p[4] - p[0];
            continue;
        }
        const uint32_t L = (uint32_t)Ls;
        uint32_t a, b;
        tm_fixed(prm, L, a, b);
        h_report->cut_fixed += L - (b - a);
        if (prm.polyg) {
            uint32_t g = 0;
            while (g < b - a && (s[b - 1 - g] | 0x20u) == 'g') ++g;
            if (g >= prm.polyg) { b -= g; h_report->cut_polyg += g; }
        }
        uint32_t a2, b2;
        tm_host_quality(u, a, b, prm.q3, prm.q5, a2, b2);
        h_report->cut_q3 += b - b2;
        if (a2 > b2) a2 = b2;
        h_report->cut_q5 += a2 - a;
        a = a2; b = b2;
        if (prm.flags & UQ_TRIM_N) {
            while (a < b && (s[a] | 0x20u) == 'n') { ++a; h_report->cut_n += 1; }
            while (b > a && (s[b - 1] | 0x20u) == 'n') { --b; h_report->cut_n += 1; }
        }
        h_window[2 * i] = a; h_window[2 * i + 1] = b;
        h_report->reads_trimmed += !(a == 0 && b == L);
        h_report->emptied += a == b && L > 0;
        h_report->bases_out += b - a;
        h_report->bytes_out += (p[4] - p[0]) - 2ull * (L - (b - a));
    }
    return 0;
}

extern "C" int uq_trim_plan(uq_ctx* ctx, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads, const uint32_t* d_window,
                            uint64_t* d_dst, uint64_t* h_out_bytes) {
    UQ_REQUIRE(ctx && d_line_start && d_dst && h_out_bytes, "uq_trim_plan: null argument");
    *h_out_bytes = 0;
    if (nreads == 0) {
        UQ_CHECK_HIP(hipMemsetAsync(d_dst, 0, 8, ctx->stream));
        return 0;
    }
    UQ_REQUIRE(d_window, "uq_trim_plan: null argument");
    UQ_REQUIRE(first_read + nreads >= first_read && first_read + nreads < (1ull << 59), "uq_trim_plan: records beyond any index");
    const uint64_t want = (nreads + 255) / 256;
    const uint32_t blocks = (uint32_t)(want < UQ_NUM_CU * TP_BLOCKS_PER_CU ? want : UQ_NUM_CU * TP_BLOCKS_PER_CU);
    trim_len_kernel<<<blocks, 256, 0, ctx->stream>>>(d_line_start, first_read, nreads, d_window, d_dst);
    UQ_LAUNCH_CHECK();
    UQ_TRY(uq_scan_exclusive_u64(ctx, d_dst, d_dst, nreads, d_dst + nreads));
    UQ_TRY(uq_read_back(ctx, ctx->h_pinned, d_dst + nreads, 8));
    UQ_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    *h_out_bytes = ctx->h_pinned[0];
    return 0;
}

extern "C" int uq_trim_plan_host(const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads, const uint32_t* h_window,
                                 uint64_t* h_dst, uint64_t* h_out_bytes) {
    UQ_REQUIRE(h_line_start && h_dst && h_out_bytes, "uq_trim_plan_host: null argument");
    UQ_REQUIRE(nreads == 0 || h_window, "uq_trim_plan_host: null argument");
    uint64_t at = 0;
    for (uint64_t i = 0; i < nreads; ++i) {
        const uint64_t* p = h_line_start + 4 * (first_read + i);
        uint64_t Ls, Lu;
        UQ_TRY(tm_host_lines("uq_trim_plan_host", p, first_read + i, Ls, Lu));
        const uint32_t a = h_window[2 * i], b = h_window[2 * i + 1];
        UQ_TRY(tm_host_window("uq_trim_plan_host", first_read + i, Ls, Lu, a, b));
        h_dst[i] = at;
        at += (p[4] - p[0]) - (Ls == Lu ? 2 * (Ls - (b - a)) : 0);
    }
    h_dst[nreads] = at;
    *h_out_bytes = at;
    return 0;
}

extern "C" int uq_trim_records(uq_ctx* ctx, const uint8_t* d_buf, uint64_t nbytes, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                               const uint32_t* d_window, const uint64_t* d_dst, uint8_t* d_out, uint64_t out_capacity, uint64_t* d_line_start_out) {
    UQ_REQUIRE(ctx, "uq_trim_records: null argument");
    if (nreads == 0) return 0;
    UQ_REQUIRE(d_buf && d_line_start && d_window && d_dst, "uq_trim_records: null argument");
    UQ_REQUIRE(first_read + nreads >= first_read && first_read + nreads < (1ull << 59), "uq_trim_records: records beyond any index");
    // the output's size, and the ends of the plan: nothing is launched on the buffers before the capacity has been checked
    uint64_t* h = ctx->h_pinned;
    void* ends;
    UQ_TRY(uq_scratch(ctx, 32, &ends));
    trim_ends_kernel<<<1, 1, 0, ctx->stream>>>(d_line_start, first_read, nreads, d_dst, (uint64_t*)ends);
    UQ_LAUNCH_CHECK();
    UQ_TRY(uq_read_back(ctx, h, ends, 32));
    UQ_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    const uint64_t size = h[1];
    UQ_REQUIRE(h[0] == 0 && size >= 4 * nreads && h[2] <= size - 4, "uq_trim_records: the plan's offsets are out of order");
    UQ_REQUIRE(h[3] <= nbytes, "uq_trim_records: the last record ends beyond the %llu bytes of the source", (unsigned long long)nbytes);
    UQ_REQUIRE(out_capacity >= size, "uq_trim_records: the output needs %llu bytes, out_capacity is %llu", (unsigned long long)size,
               (unsigned long long)out_capacity);
    UQ_REQUIRE(d_out, "uq_trim_records: null argument");
    const uint32_t mis = (uint32_t)((uintptr_t)d_out & 15u);
    const uint64_t ntiles = (size + mis + TC_TILE - 1) / TC_TILE;
    UQ_REQUIRE(ntiles < (1ull << 31), "uq_trim_records: more than 2^31 output tiles");
    void* ws;
    UQ_TRY(uq_scratch(ctx, (ntiles + 1) * 8, &ws));
    trim_origin_kernel<<<(uint32_t)((ntiles + 1 + 255) / 256), 256, 0, ctx->stream>>>(d_dst, nreads, size, mis, ntiles, (uint64_t*)ws);
    UQ_LAUNCH_CHECK();
    trim_copy_kernel<<<(uint32_t)ntiles, TC_THREADS, 0, ctx->stream>>>(d_buf, d_line_start, first_read, nreads, d_window, d_dst, size, d_out,
                                                                       (const uint64_t*)ws);
    UQ_LAUNCH_CHECK();
    if (d_line_start_out) {
        const uint64_t want = (nreads + 255) / 256;
        const uint32_t blocks = (uint32_t)(want < UQ_NUM_CU * TP_BLOCKS_PER_CU ? want : UQ_NUM_CU * TP_BLOCKS_PER_CU);
        trim_index_kernel<<<blocks, 256, 0, ctx->stream>>>(d_line_start, first_read, nreads, d_window, d_dst, d_line_start_out);
        UQ_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int uq_trim_records_host(const uint8_t* h_buf, uint64_t nbytes, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                                    const uint32_t* h_window, const uint64_t* h_dst, uint8_t* h_out, uint64_t out_capacity, uint64_t* h_line_start_out) {
    if (nreads == 0) return 0;
    UQ_REQUIRE(h_buf && h_line_start && h_window && h_dst, "uq_trim_records_host: null argument");
    UQ_REQUIRE(out_capacity >= h_dst[nreads], "uq_trim_records_host: the output needs %llu bytes, out_capacity is %llu",
               (unsigned long long)h_dst[nreads], (unsigned long long)out_capacity);
    UQ_REQUIRE(h_out, "uq_trim_records_host: null argument");
    for (uint64_t i = 0; i < nreads; ++i) {
        const uint64_t* p = h_line_start + 4 * (first_read + i);
        uint64_t Ls, Lu;
        UQ_TRY(tm_host_lines("uq_trim_records_host", p, first_read + i, Ls, Lu));
        UQ_REQUIRE(p[4] <= nbytes, "uq_trim_records_host: record %llu lies outside the source", (unsigned long long)(first_read + i));
        const uint32_t a = h_window[2 * i], b = h_window[2 * i + 1];
        UQ_TRY(tm_host_window("uq_trim_records_host", first_read + i, Ls, Lu, a, b));
        const uint64_t len = (p[4] - p[0]) - (Ls == Lu ? 2 * (Ls - (b - a)) : 0);
        UQ_REQUIRE(h_dst[i + 1] >= h_dst[i] && h_dst[i + 1] - h_dst[i] == len && h_dst[i + 1] <= h_dst[nreads],
                   "uq_trim_records_host: record %llu: the plan does not hold its %llu bytes", (unsigned long long)(first_read + i), (unsigned long long)len);
        uint8_t* o = h_out + h_dst[i];
        uint64_t at = 0;
        if (h_line_start_out) h_line_start_out[4 * i] = h_dst[i];
        memcpy(o, h_buf + p[0], p[1] - p[0]); at += p[1] - p[0];                            // qn '\n'
        if (h_line_start_out) h_line_start_out[4 * i + 1] = h_dst[i] + at;
        if (Ls != Lu) {
            memcpy(o + at, h_buf + p[1], p[4] - p[1]);                                       // the rest as it is
            if (h_line_start_out) { h_line_start_out[4 * i + 2] = h_dst[i] + (p[2] - p[0]); h_line_start_out[4 * i + 3] = h_dst[i] + (p[3] - p[0]); }
            continue;
        }
        memcpy(o + at, h_buf + p[1] + a, b - a); at += b - a;                                 // s[a:b]
        o[at++] = '\n';
        if (h_line_start_out) h_line_start_out[4 * i + 2] = h_dst[i] + at;
        memcpy(o + at, h_buf + p[2], p[3] - p[2]); at += p[3] - p[2];                         // p '\n'
        if (h_line_start_out) h_line_start_out[4 * i + 3] = h_dst[i] + at;
        memcpy(o + at, h_buf + p[3] + a, b - a); at += b - a;                                 // u[a:b]
        o[at++] = '\n';
    }
    if (h_line_start_out) h_line_start_out[4 * nreads] = h_dst[nreads];
    return 0;
}
