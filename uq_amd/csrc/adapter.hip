// adapter.hip -- 3' adapter detection (`--adapter`).  An extension: the reference stores every read as it is given.
//
// uq_adapter_mark narrows every record's window [a, b) to [a, p*) for the leftmost position p* at which the adapter matches what is left of
// the window with few enough mismatches (the definition is in include/uqhip.h).  The plan and the copy are uq_trim_plan / uq_trim_records.
//
// adapter_mark_kernel takes its stager from trim_mark_kernel (trim.hip; a copy, not shared): persistent workgroups walk tiles of R consecutive
// records, a tile is one contiguous span copied to LDS with coalesced 16-byte loads (the next tile's bytes are in flight, its bounds were
// asked for a turn earlier), P lanes (a power of two, 4 .. 16) share a record.  A record is then handled in two phases:
//   pack   a lane turns 8 bytes of the window into 16 bits of 2-bit codes ((byte >> 1) & 3: A 0, C 1, T 2, G 3 in either case) and 8 "not ACGT"
//          bits spread to the same 2-bit stride, both gathered with shifts and masks (no byte loop), and stores them in a packed area in LDS;
//   scan   the lanes of a record take the positions a + lane, a + lane + P, ... in rising order.  A position is 64 bases of codes and of
//          invalid bits at bit offset 2 (p - a) -- funnel shifts over five dwords, or 32 bases over three when no adapter is longer than 32 --,
//          XORed with the adapter's packed codes (kernel arguments), folded with (x | x >> 1) & 0x55.., ORed with the invalid bits, masked to
//          m(p) bases and counted.  After every step a ballot over the record's lanes gives the first candidate; a record that has one is
//          walked no further.
// A tile beyond the stage is read straight from HBM and the stage holds the packed form instead: its records take a half-wave each, except
// those with a line beyond AD_LONG bytes, which the WHOLE workgroup walks in segments of AD_SEG positions packed with the 63 bases behind
// them -- never one thread along a line.  The report is kept as per-lane sums: one atomic per field per workgroup at the end.
#include "common.h"
#include "swar.h"

namespace {
enum { AR_READS_IN = 0, AR_BASES_IN, AR_BASES_OUT, AR_READS_CUT, AR_FULL, AR_PARTIAL, AR_MATE2, AR_EMPTIED, AR_LEN_MISMATCH, AR_WORDS };
static_assert(sizeof(uq_adapter_report) == AR_WORDS * 8, "the report is nine u64 words");
static_assert(sizeof(uq_adapter_params) == 160, "eight u32 words and two sequences of 64 bytes");

constexpr int AD_THREADS = 256;
constexpr int AD_NV = 5;                          // 16-byte loads per lane per tile
constexpr uint32_t AD_CAP = AD_NV * 256 * 16;     // staging bytes per tile (20 KiB)
constexpr uint32_t AD_PAD = 16;                   // bytes in front of the stage
constexpr uint32_t AD_RMAX = 64;                  // records per tile, upper bound (4 * AD_RMAX + 1 <= 2 * AD_THREADS)
constexpr uint32_t AD_LONG = 4096;                // in a tile beyond the stage: a line longer than this is walked by the whole workgroup, the others by a half-wave
constexpr uint32_t AD_SEG = 16384;                // positions of a long line the workgroup scans between two packs
// the packed areas, in dwords of 16 bases.  A scan reads up to four dwords beyond the one its position lies in.
constexpr uint32_t AD_PK_REC = 10;                // staged tiles: record j's area begins at (its offset in the stage >> 5) + AD_PK_REC * j
constexpr uint32_t AD_PK = ((AD_CAP + 16) >> 5) + AD_PK_REC * AD_RMAX + 16;      // a record of Ls bases needs Ls / 16 + 5 and is 2 Ls + 4 bytes at least
constexpr uint32_t AD_PK_HALF = AD_LONG / 16 + 16;                               // tiles beyond the stage: a half-wave's area, in the stage
constexpr uint32_t AD_PK_SEG = (AD_SEG + 64) / 16 + 16;                          // ... and the workgroup's, for one segment
static_assert(2 * 8 * AD_PK_HALF * 4 <= AD_CAP && 2 * AD_PK_SEG * 4 <= AD_CAP, "the packed form of a tile beyond the stage fits the stage");
constexpr uint64_t AD_H = 0x8080808080808080ull;
constexpr uint32_t AD_NONE = 0xFFFFFFFFu;

// high bit of every byte of w that equals the byte of `pat` when its 0x20 bit is set (a letter of either case); exact, no carries between bytes
__device__ __forceinline__ uint64_t ad_eq_bits(uint64_t w, uint64_t pat) {
    const uint64_t x = (w | 0x2020202020202020ull) ^ pat;
    return ~(((x & ~AD_H) + ~AD_H) | x | ~AD_H);
}
// 8 bytes -> their 2-bit codes in bits 0 .. 15 and, in bits 16 .. 31, bit 2 j set where byte j is no letter of ACGT
__device__ __forceinline__ uint32_t ad_pack8(uint64_t w) {
    const uint64_t ok = ad_eq_bits(w, 0x6161616161616161ull) | ad_eq_bits(w, 0x6363636363636363ull) | ad_eq_bits(w, 0x6767676767676767ull) |
                        ad_eq_bits(w, 0x7474747474747474ull);
    uint64_t c = (w >> 1) & 0x0303030303030303ull;
    c = (c | (c >> 6)) & 0x000F000F000F000Full;
    c = (c | (c >> 12)) & 0x000000FF000000FFull;
    c = (c | (c >> 24)) & 0xFFFFull;
    uint64_t v = ((~ok & AD_H) >> 7);
    v = (v | (v >> 6)) & 0x0005000500050005ull;
    v = (v | (v >> 12)) & 0x0000005500000055ull;
    v = (v | (v >> 24)) & 0x5555ull;
    return (uint32_t)c | ((uint32_t)v << 16);
}

// the bytes pos .. pos + 7 of a line in HBM; bytes outside the line are zero
struct AdHbmLine {
    const uint8_t* p; uint64_t L;
    __device__ __forceinline__ uint64_t get8(uint64_t pos) const {
        uint64_t w = 0;
        if (pos + 8 <= L) __builtin_memcpy(&w, p + pos, 8);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const uint64_t q = pos + j; if (q < L) w |= (uint64_t)p[q] << (8 * j); }
        }
        return w;
    }
};

// an adapter: its bases as 2-bit codes, base j in bits 2 j of (lo, hi), its length, and what a candidate needs
struct AdSeq { uint64_t lo, hi; uint32_t len; };

// is `rel` (a position relative to the first packed base) a candidate, m bases compared?  pc / pv: the packed codes / invalid bits
template <bool WIDE>
__device__ __forceinline__ bool ad_test(const uint32_t* pc, const uint32_t* pv, uint32_t rel, uint32_t m, const AdSeq& A, uint32_t err) {
    const uint32_t d = rel >> 4, sh = (rel & 15u) * 2u;
    const uint32_t c0 = pc[d], c1 = pc[d + 1], c2 = pc[d + 2], v0 = pv[d], v1 = pv[d + 1], v2 = pv[d + 2];
    const uint64_t C = (uint64_t)__builtin_amdgcn_alignbit(c1, c0, sh) | ((uint64_t)__builtin_amdgcn_alignbit(c2, c1, sh) << 32);
    const uint64_t V = (uint64_t)__builtin_amdgcn_alignbit(v1, v0, sh) | ((uint64_t)__builtin_amdgcn_alignbit(v2, v1, sh) << 32);
    const uint64_t x = C ^ A.lo;
    const uint64_t mm = ((x | (x >> 1)) & 0x5555555555555555ull) | V;
    const uint64_t mask = m >= 32 ? ~0ull : ((1ull << (2 * m)) - 1);
    uint32_t cnt = (uint32_t)__popcll(mm & mask);
    if (WIDE) {
        const uint32_t c3 = pc[d + 3], c4 = pc[d + 4], v3 = pv[d + 3], v4 = pv[d + 4];
        const uint64_t C1 = (uint64_t)__builtin_amdgcn_alignbit(c3, c2, sh) | ((uint64_t)__builtin_amdgcn_alignbit(c4, c3, sh) << 32);
        const uint64_t V1 = (uint64_t)__builtin_amdgcn_alignbit(v3, v2, sh) | ((uint64_t)__builtin_amdgcn_alignbit(v4, v3, sh) << 32);
        const uint64_t x1 = C1 ^ A.hi;
        const uint64_t mm1 = ((x1 | (x1 >> 1)) & 0x5555555555555555ull) | V1;
        const uint64_t mask1 = m <= 32 ? 0ull : (m >= 64 ? ~0ull : ((1ull << (2 * m - 64)) - 1));
        cnt += (uint32_t)__popcll(mm1 & mask1);
    }
    return cnt * 100u <= m * err;                 // cnt <= (m * err) / 100 by integer division
}

// nl lanes of one wave (a power of two up to 32, aligned) scan the positions [0, npos) of a window of n bases whose packed form begins at
// pc / pv: the first candidate, AD_NONE if there is none.  Every lane of the group runs the same trips and gets the answer.
template <bool WIDE>
__device__ __forceinline__ uint32_t ad_scan_lanes(uint32_t l, uint32_t nl, const uint32_t* pc, const uint32_t* pv, uint32_t n, uint32_t npos,
                                                  const AdSeq& A, uint32_t err) {
    const uint32_t g0 = lane_id() & ~(nl - 1);
    for (uint32_t base = 0; base < npos; base += nl) {
        const uint32_t r = base + l;
        bool hit = false;
        if (r < npos) { const uint32_t left = n - r; hit = ad_test<WIDE>(pc, pv, r, left < A.len ? left : A.len, A, err); }
        const uint64_t m = (__ballot(hit) >> g0) & ((1ull << nl) - 1);
        if (m) return base + (uint32_t)__ffsll((long long)m) - 1u;
    }
    return AD_NONE;
}

// the smallest v over the workgroup, through `red` (AD_THREADS / 64 words of LDS); every thread of the block makes the call
__device__ __forceinline__ uint32_t ad_block_min(uint32_t v, uint32_t* red) {
    v = wave_min(v);
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t m = red[0];
    for (int w = 1; w < AD_THREADS / 64; ++w) m = red[w] < m ? red[w] : m;
    __syncthreads();
    return m;
}

struct AdAcc {
    uint64_t bases_in = 0, bases_out = 0;
    uint32_t reads = 0, full = 0, partial = 0, mate2 = 0, emptied = 0, mismatch = 0;      // < 2^32: a lane sees fewer than 2^32 records
    // a record whose window was [a, b) and is [a, b2) now: cut at b2 by an adapter of `len` bases when b2 < b or `cut`
    __device__ __forceinline__ void record(uint32_t a, uint32_t b, uint32_t cut_at, uint32_t len, bool second) {
        ++reads; bases_in += b - a;
        if (cut_at == AD_NONE) { bases_out += b - a; return; }
        bases_out += cut_at;
        const bool is_full = b - a - cut_at >= len;
        full += is_full; partial += !is_full; mate2 += second;
        emptied += cut_at == 0;                   // (a candidate needs overlap >= 1 bases: the window was not empty)
    }
    __device__ __forceinline__ void unequal(uint64_t Ls) { ++reads; ++mismatch; bases_in += Ls; bases_out += Ls; }
};

template <bool WIDE>
__global__ __launch_bounds__(AD_THREADS) void adapter_mark_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ ls, uint64_t first, uint64_t n,
                                                                  AdSeq A1, AdSeq A2, uint32_t overlap, uint32_t err, uint32_t flags,
                                                                  uint32_t* __restrict__ window, unsigned long long* __restrict__ report) {
    __shared__ __align__(16) uint8_t stage_raw[AD_PAD + AD_CAP + 32];
    __shared__ uint32_t pk_c[AD_PK], pk_v[AD_PK];
    __shared__ uint32_t meta[4 * AD_RMAX + 4];
    __shared__ uint32_t cfg[2];
    __shared__ uint32_t redm[AD_THREADS / 64];
    __shared__ uint64_t red[AD_THREADS / 64][8];
    uint8_t* const stage = stage_raw + AD_PAD;
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const bool fresh = flags & UQ_ADAPTER_FRESH, paired = flags & UQ_ADAPTER_PAIRED;
    // the tile geometry is decided here from the shard's average record length (no round trip in front of the launch, as in trim.hip)
    if (tid == 0) {
        const uint64_t avg = (ls[4 * (first + n)] - ls[4 * first]) / n + 1;
        uint64_t R = (AD_CAP - 64) / (avg + avg / 8 + 1);
        R = R > AD_RMAX ? AD_RMAX : (R < 1 ? 1 : R);
        uint32_t P = 16;
        while (P > 1 && P * (uint32_t)R > AD_THREADS) P >>= 1;      // a power of two: the lanes of a record share a ballot
        cfg[0] = (uint32_t)R; cfg[1] = P;
    }
    __syncthreads();
    const uint32_t R = __builtin_amdgcn_readfirstlane(cfg[0]), P = __builtin_amdgcn_readfirstlane(cfg[1]);
    const uint64_t ntiles = (n + R - 1) / R;
    const uint32_t rr = tid / P, pp = tid & (P - 1);
    AdAcc acc;

    const uint64_t S = gridDim.x;
    struct Bounds { uint64_t g0, g1; };
    struct Regs { uint4 v[AD_NV]; uint64_t m0, m1; uint64_t g0; uint32_t skew, nvec, Rt; bool exists, staged; };
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
        for (int u = 0; u < AD_NV; ++u) x.v[u] = make_uint4(0, 0, 0, 0);
        if (!x.exists) return x;
        x.Rt = (uint32_t)((n - tt * R) < R ? (n - tt * R) : R);
        const uint64_t a0 = ((uint64_t)(uintptr_t)buf + b.g0) & ~uint64_t(15);
        x.skew = (uint32_t)(((uint64_t)(uintptr_t)buf + b.g0) - a0);
        const uint64_t span = b.g1 - b.g0 + x.skew;
        x.staged = span + 16 <= AD_CAP;
        if (!x.staged) return x;
        x.nvec = (uint32_t)((span + 15) >> 4);
        const uint4* src = (const uint4*)(buf + ((int64_t)b.g0 - (int64_t)x.skew));      // aligned vectors that hold at least one byte of the span
#pragma unroll
        for (int u = 0; u < AD_NV; ++u) { const uint32_t i = u * AD_THREADS + tid; if (i < x.nvec) x.v[u] = src[i]; }
        const uint64_t* lsp = ls + 4 * (first + tt * R);
        if (tid <= 4 * x.Rt) x.m0 = lsp[tid];
        if (tid + AD_THREADS <= 4 * x.Rt) x.m1 = lsp[tid + AD_THREADS];
        return x;
    };
    // a record's window as it is received: a <= b <= Ls is the caller's contract; it is clamped so that nothing outside the line is read
    auto window_in = [&](uint64_t i, uint32_t Ls, uint32_t& a, uint32_t& b) {
        a = 0; b = Ls;
        if (!fresh) {
            b = window[2 * i + 1]; b = b < Ls ? b : Ls;
            a = window[2 * i]; a = a < b ? a : b;
        }
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
            if (tid + AD_THREADS <= 4 * Rt) meta[tid + AD_THREADS] = (uint32_t)(cur.m1 - cur.g0) + cur.skew;
#pragma unroll
            for (int u = 0; u < AD_NV; ++u) { const uint32_t i = u * AD_THREADS + tid; if (i < cur.nvec) ((uint4*)stage)[i] = cur.v[u]; }
        }
        __syncthreads();
        const bool staged = cur.staged;
        cur = issue(t + S, b_next);          // the next tile's loads fly while this one is scanned
        b_next = b_nn;
        if (staged) {
            uint32_t a = 0, b = 0, Ls = 0, Lu = 0, pk0 = 0;
            const bool have = rr < Rt;
            if (have) {
                const uint32_t o = meta[4 * rr], s = meta[4 * rr + 1], e1 = meta[4 * rr + 2], q = meta[4 * rr + 3], e2 = meta[4 * rr + 4];
                Ls = e1 - s - 1; Lu = e2 - q - 1;
                pk0 = (o >> 5) + AD_PK_REC * rr;
                if (Ls == Lu) {
                    window_in(r0 + rr, Ls, a, b);
                    const uint32_t chunks = (b - a + 7) >> 3;
                    for (uint32_t k = pp; k < chunks; k += P) {
                        uint32_t lo, hi;
                        lds_window8(stage, (int32_t)(s + a + 8 * k), lo, hi);
                        const uint32_t w = ad_pack8((uint64_t)lo | ((uint64_t)hi << 32));
                        ((uint16_t*)pk_c)[2 * pk0 + k] = (uint16_t)w; ((uint16_t*)pk_v)[2 * pk0 + k] = (uint16_t)(w >> 16);
                    }
                }
            }
            __syncthreads();
            if (have) {                      // (the same for the P lanes of a record: they ballot among themselves only)
                if (Ls == Lu) {
                    const bool second = paired && ((first + r0 + rr) & 1);
                    const AdSeq A = second ? A2 : A1;
                    const uint32_t nb = b - a;
                    const uint32_t hit = nb >= overlap ? ad_scan_lanes<WIDE>(pp, P, pk_c + pk0, pk_v + pk0, nb, nb - overlap + 1, A, err) : AD_NONE;
                    if (pp == 0) {
                        window[2 * (r0 + rr)] = a; window[2 * (r0 + rr) + 1] = hit == AD_NONE ? b : a + hit;
                        acc.record(a, b, hit, A.len, second);
                    }
                } else if (pp == 0) {
                    window[2 * (r0 + rr)] = 0; window[2 * (r0 + rr) + 1] = Ls;
                    acc.unequal(Ls);
                }
            }
        } else {
            // a span beyond the stage (a long read in it, or a run of longer-than-average ones): straight from HBM, the packed form in the
            // stage.  Records whose lines are at most AD_LONG bytes take a half-wave each, eight at a time; a record with longer lines is
            // walked by the whole workgroup.
            const uint64_t* lsp = ls + 4 * (first + r0);
            uint32_t* const sp = (uint32_t*)stage_raw;
            for (uint32_t rb = 0; rb < Rt; rb += 2 * (AD_THREADS / 64)) {      // (the same trips for every thread: the barriers are met by all)
                const uint32_t hw = 2 * wave + (lane >> 5), r = rb + hw, hl = lane & 31u;
                uint32_t* const pc = sp + hw * AD_PK_HALF;
                uint32_t* const pv = sp + (2 * (AD_THREADS / 64) + hw) * AD_PK_HALF;
                uint64_t s = 0, Ls = 0, Lu = 0;
                uint32_t a = 0, b = 0;
                bool mine = false;
                if (r < Rt) {
                    const uint64_t* p = lsp + 4 * r;
                    s = p[1];
                    Ls = p[2] - s - 1; Lu = p[4] - p[3] - 1;
                    mine = Ls != Lu || Ls <= AD_LONG;
                    if (mine && Ls == Lu) {
                        window_in(r0 + r, (uint32_t)Ls, a, b);
                        const AdHbmLine f{buf + s, Ls};
                        const uint32_t chunks = (b - a + 7) >> 3;
                        for (uint32_t k = hl; k < chunks; k += 32) {
                            const uint32_t w = ad_pack8(f.get8((uint64_t)a + 8 * k));
                            ((uint16_t*)pc)[k] = (uint16_t)w; ((uint16_t*)pv)[k] = (uint16_t)(w >> 16);
                        }
                    }
                }
                __syncthreads();
                if (mine) {                  // (the same for the 32 lanes of a half-wave)
                    if (Ls == Lu) {
                        const bool second = paired && ((first + r0 + r) & 1);
                        const AdSeq A = second ? A2 : A1;
                        const uint32_t nb = b - a;
                        const uint32_t hit = nb >= overlap ? ad_scan_lanes<WIDE>(hl, 32u, pc, pv, nb, nb - overlap + 1, A, err) : AD_NONE;
                        if (hl == 0) {
                            window[2 * (r0 + r)] = a; window[2 * (r0 + r) + 1] = hit == AD_NONE ? b : a + hit;
                            acc.record(a, b, hit, A.len, second);
                        }
                    } else if (hl == 0) {
                        window[2 * (r0 + r)] = 0; window[2 * (r0 + r) + 1] = (uint32_t)Ls;
                        acc.unequal(Ls);
                    }
                }
                __syncthreads();
            }
            for (uint32_t r = 0; r < Rt; ++r) {
                const uint64_t* p = lsp + 4 * r;
                const uint64_t s = p[1], Ls = p[2] - s - 1, Lu = p[4] - p[3] - 1;
                if (Ls != Lu || Ls <= AD_LONG) continue;                       // (the same for every thread: no barrier is skipped by some)
                uint32_t a, b;
                window_in(r0 + r, (uint32_t)Ls, a, b);
                const bool second = paired && ((first + r0 + r) & 1);
                const AdSeq A = second ? A2 : A1;
                const AdHbmLine f{buf + s, Ls};
                const uint32_t nb = b - a;
                uint32_t* const pc = sp;
                uint32_t* const pv = sp + AD_PK_SEG;
                uint32_t hit = AD_NONE;
                if (nb >= overlap) {
                    const uint64_t npos_all = (uint64_t)nb - overlap + 1;
                    for (uint64_t s0 = 0; s0 < npos_all; s0 += AD_SEG) {
                        const uint32_t npos = (uint32_t)(npos_all - s0 < AD_SEG ? npos_all - s0 : AD_SEG);
                        const uint64_t left = (uint64_t)nb - s0;
                        const uint32_t nbases = (uint32_t)(left < npos + 63u ? left : npos + 63u);
                        const uint32_t chunks = (nbases + 7) >> 3;
                        for (uint32_t k = tid; k < chunks; k += AD_THREADS) {
                            const uint32_t w = ad_pack8(f.get8((uint64_t)a + s0 + 8 * k));
                            ((uint16_t*)pc)[k] = (uint16_t)w; ((uint16_t*)pv)[k] = (uint16_t)(w >> 16);
                        }
                        __syncthreads();
                        uint32_t found = AD_NONE;
                        for (uint32_t rel = tid; rel < npos && found == AD_NONE; rel += AD_THREADS) {
                            const uint64_t lf = left - rel;
                            if (ad_test<WIDE>(pc, pv, rel, lf < A.len ? (uint32_t)lf : A.len, A, err)) found = (uint32_t)(s0 + rel);
                        }
                        hit = ad_block_min(found, redm);                       // (its barriers also keep the next pack behind this scan)
                        if (hit != AD_NONE) break;
                    }
                }
                if (tid == 0) {
                    window[2 * (r0 + r)] = a; window[2 * (r0 + r) + 1] = hit == AD_NONE ? b : a + hit;
                    acc.record(a, b, hit, A.len, second);
                }
            }
        }
        __syncthreads();
    }
    // the report: per-lane sums -> one atomic per field per workgroup
    uint64_t f[8] = {acc.reads, acc.bases_in, acc.bases_out, acc.full, acc.partial, acc.mate2, acc.emptied, acc.mismatch};
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) { f[k] = wave_sum(f[k]); if (lane == 0) red[wave][k] = f[k]; }
    __syncthreads();
    if (tid < 9) {
        // thread 8 adds reads_cut = full + partial
        const uint32_t k0 = tid < 8 ? tid : 3u, k1 = tid < 8 ? tid : 4u;
        uint64_t v = 0;
        for (int w = 0; w < AD_THREADS / 64; ++w) v += red[w][k0] + (k1 != k0 ? red[w][k1] : 0);
        const uint32_t field = tid == 8 ? AR_READS_CUT : (tid < 3 ? tid : tid + 1);
        if (v) atomicAdd(report + field, (unsigned long long)v);
    }
}

// classes 0 .. 3 (A C G T) -> the kernel's codes ((byte >> 1) & 3 of the letter: A 0, C 1, T 2, G 3), packed
AdSeq ad_pack_seq(const uint8_t* seq, uint32_t len) {
    AdSeq A{0, 0, len};
    for (uint32_t j = 0; j < len; ++j) {
        const uint64_t c = seq[j] ^ (seq[j] >> 1);
        if (j < 32) A.lo |= c << (2 * j); else A.hi |= c << (2 * (j - 32));
    }
    return A;
}

int ad_check_params(const char* who, const uq_adapter_params* p) {
    UQ_REQUIRE(p, "%s: null argument", who);
    UQ_REQUIRE((p->flags & ~(UQ_ADAPTER_FRESH | UQ_ADAPTER_PAIRED)) == 0, "%s: unknown flag bits 0x%x", who, p->flags);
    UQ_REQUIRE(p->reserved[0] == 0 && p->reserved[1] == 0 && p->reserved[2] == 0, "%s: reserved words must be 0", who);
    UQ_REQUIRE(p->len1 >= 1 && p->len1 <= UQ_ADAPTER_MAX, "%s: len1 %u outside 1..%d", who, p->len1, UQ_ADAPTER_MAX);
    UQ_REQUIRE(p->len2 <= UQ_ADAPTER_MAX, "%s: len2 %u > %d", who, p->len2, UQ_ADAPTER_MAX);
    const bool paired = p->flags & UQ_ADAPTER_PAIRED;
    UQ_REQUIRE(!paired || p->len2 >= 1, "%s: len2 is 0 with UQ_ADAPTER_PAIRED", who);
    for (uint32_t j = 0; j < p->len1; ++j) UQ_REQUIRE(p->seq1[j] <= 3, "%s: seq1[%u] = %u is no class of A, C, G, T (0..3)", who, j, p->seq1[j]);
    for (uint32_t j = 0; j < p->len2; ++j) UQ_REQUIRE(p->seq2[j] <= 3, "%s: seq2[%u] = %u is no class of A, C, G, T (0..3)", who, j, p->seq2[j]);
    const uint32_t shortest = paired && p->len2 < p->len1 ? p->len2 : p->len1;
    UQ_REQUIRE(p->overlap >= 1 && p->overlap <= shortest, "%s: overlap %u outside 1..%u (the shorter sequence)", who, p->overlap, shortest);
    UQ_REQUIRE(p->err_pct <= 30, "%s: err_pct %u > 30", who, p->err_pct);
    return 0;
}

// the QC tables' class of a byte: A 0, C 1, G 2, T 3 in either case, N 4, anything else 5
uint32_t ad_cls(uint8_t c) {
    switch (c | 0x20u) {
        case 'a': return 0; case 'c': return 1; case 'g': return 2; case 't': return 3; case 'n': return 4;
        default: return 5;
    }
}

// the workgroups of kernel k that a CU holds at once, at most 4: from its register count (VGPRs are handed out in eights, 512 a SIMD lane;
// the count is cached in the context, as the pack kernels' is -- pack.hip says why the occupancy call is not asked) and its LDS
int ad_resident_per_cu(uq_ctx* ctx, const void* k, uint32_t& per_cu) {
    int regs = 0;
    for (int i = 0; i < ctx->kreg_n; ++i) if (ctx->kreg_key[i] == k) regs = ctx->kreg_val[i];
    if (regs == 0) {
        hipFuncAttributes fa;
        UQ_CHECK_HIP(hipFuncGetAttributes(&fa, k));
        regs = fa.numRegs > 0 ? fa.numRegs : 128;
        const int slot = ctx->kreg_n < 8 ? ctx->kreg_n++ : 7;
        ctx->kreg_key[slot] = k; ctx->kreg_val[slot] = regs;
    }
    const uint32_t alloc = ((uint32_t)regs + 7) & ~7u;
    uint32_t waves_per_simd = 512 / alloc;                       // a workgroup of AD_THREADS is one wave on each of the four SIMDs
    const uint32_t by_lds = (160 * 1024) / (AD_PAD + AD_CAP + 32 + 8 * AD_PK + 4 * (4 * AD_RMAX + 4) + 512);
    per_cu = waves_per_simd < by_lds ? waves_per_simd : by_lds;
    per_cu = per_cu > 4 ? 4 : (per_cu < 1 ? 1 : per_cu);
    return 0;
}
}  // namespace

extern "C" int uq_adapter_report_init(uq_ctx* ctx, uq_adapter_report* d_report) {
    UQ_REQUIRE(ctx && d_report, "uq_adapter_report_init: null argument");
    UQ_CHECK_HIP(hipMemsetAsync(d_report, 0, sizeof(uq_adapter_report), ctx->stream));
    return 0;
}

extern "C" int uq_adapter_report_init_host(uq_adapter_report* h_report) {
    UQ_REQUIRE(h_report, "uq_adapter_report_init_host: null argument");
    memset(h_report, 0, sizeof(uq_adapter_report));
    return 0;
}

extern "C" int uq_adapter_mark(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                               const uq_adapter_params* h_params, uint32_t* d_window, uq_adapter_report* d_report) {
    UQ_REQUIRE(ctx && d_line_start && d_report, "uq_adapter_mark: null argument");
    UQ_TRY(ad_check_params("uq_adapter_mark", h_params));
    UQ_REQUIRE(((uintptr_t)d_report & 7) == 0, "uq_adapter_mark: d_report must be 8-byte aligned");
    if (nreads == 0) return 0;
    UQ_REQUIRE(d_buf && d_window, "uq_adapter_mark: null argument");
    UQ_REQUIRE(((uintptr_t)d_window & 3) == 0, "uq_adapter_mark: d_window must be 4-byte aligned");
    UQ_REQUIRE(first_read + nreads >= first_read && first_read + nreads < (1ull << 59), "uq_adapter_mark: records beyond any index");
    const uq_adapter_params& prm = *h_params;
    const bool paired = prm.flags & UQ_ADAPTER_PAIRED;
    const AdSeq A1 = ad_pack_seq(prm.seq1, prm.len1);
    const AdSeq A2 = paired ? ad_pack_seq(prm.seq2, prm.len2) : A1;
    // persistent workgroups with their tiles dealt in turn: exactly as many as are resident at once (a fourth per CU, which the registers do
    // not admit, would hold a quarter of the tiles and run them as a second, quarter-full round); a tile holds >= 1 record, surplus
    // workgroups leave at once
    const bool wide = A1.len > 32 || A2.len > 32;
    uint32_t per_cu;
    UQ_TRY(ad_resident_per_cu(ctx, wide ? (const void*)adapter_mark_kernel<true> : (const void*)adapter_mark_kernel<false>, per_cu));
    const uint32_t blocks = (uint32_t)(nreads < UQ_NUM_CU * per_cu ? nreads : UQ_NUM_CU * per_cu);
    if (wide)
        adapter_mark_kernel<true><<<blocks, AD_THREADS, 0, ctx->stream>>>(d_buf, d_line_start, first_read, nreads, A1, A2, prm.overlap, prm.err_pct, prm.flags,
                                                                          d_window, (unsigned long long*)d_report);
    else
        adapter_mark_kernel<false><<<blocks, AD_THREADS, 0, ctx->stream>>>(d_buf, d_line_start, first_read, nreads, A1, A2, prm.overlap, prm.err_pct, prm.flags,
                                                                           d_window, (unsigned long long*)d_report);
    UQ_LAUNCH_CHECK();
    return 0;
}

extern "C" int uq_adapter_mark_host(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                                    const uq_adapter_params* h_params, uint32_t* h_window, uq_adapter_report* h_report) {
    UQ_REQUIRE(h_line_start && h_report, "uq_adapter_mark_host: null argument");
    UQ_TRY(ad_check_params("uq_adapter_mark_host", h_params));
    if (nreads == 0) return 0;
    UQ_REQUIRE(h_buf && h_window, "uq_adapter_mark_host: null argument");
    const uq_adapter_params& prm = *h_params;
    // every record and every window handed in is checked before anything is written: an error leaves windows and report as they were
    for (uint64_t i = 0; i < nreads; ++i) {
        const uint64_t r = first_read + i;
        const uint64_t* p = h_line_start + 4 * r;
        UQ_REQUIRE(p[1] > p[0] && p[2] > p[1] && p[3] > p[2] && p[4] > p[3], "uq_adapter_mark_host: record %llu: line starts out of order", (unsigned long long)r);
        UQ_REQUIRE(p[2] - p[1] <= 0xFFFFFFFFull && p[4] - p[3] <= 0xFFFFFFFFull, "uq_adapter_mark_host: record %llu: a line of 2^32 bytes or more",
                   (unsigned long long)r);
        const uint64_t Ls = p[2] - p[1] - 1, Lu = p[4] - p[3] - 1;
        if (Ls == Lu && !(prm.flags & UQ_ADAPTER_FRESH))
            UQ_REQUIRE(h_window[2 * i] <= h_window[2 * i + 1] && h_window[2 * i + 1] <= Ls,
                       "uq_adapter_mark_host: record %llu: the window (%u, %u) does not lie in a line of %llu bytes", (unsigned long long)r, h_window[2 * i],
                       h_window[2 * i + 1], (unsigned long long)Ls);
    }
    for (uint64_t i = 0; i < nreads; ++i) {
        const uint64_t r = first_read + i;
        const uint64_t* p = h_line_start + 4 * r;
        const uint64_t Ls = p[2] - p[1] - 1, Lu = p[4] - p[3] - 1;
        const uint8_t* s = h_buf + p[1];
        h_report->reads_in += 1;
        if (Ls != Lu) {
            h_window[2 * i] = 0; h_window[2 * i + 1] = (uint32_t)Ls;
            h_report->len_mismatch += 1; h_report->bases_in += Ls; h_report->bases_out += Ls;
            continue;
        }
        uint32_t a = 0, b = (uint32_t)Ls;
        if (!(prm.flags & UQ_ADAPTER_FRESH)) {
            a = h_window[2 * i]; b = h_window[2 * i + 1];
        }
        const bool second = (prm.flags & UQ_ADAPTER_PAIRED) && (r & 1);
        const uint8_t* A = second ? prm.seq2 : prm.seq1;
        const uint32_t La = second ? prm.len2 : prm.len1;
        uint32_t cut = b;
        bool found = false, full = false;
        for (uint32_t pos = a; pos < b && !found; ++pos) {
            const uint32_t m = b - pos < La ? b - pos : La;
            if (m < prm.overlap) break;                                        // (m only falls from here on)
            uint32_t mis = 0;
            for (uint32_t j = 0; j < m; ++j) mis += ad_cls(s[pos + j]) != A[j];
            if (mis <= (m * prm.err_pct) / 100) { found = true; cut = pos; full = m == La; }
        }
        h_window[2 * i] = a; h_window[2 * i + 1] = cut;
        h_report->bases_in += b - a; h_report->bases_out += cut - a;
        if (found) {
            h_report->reads_cut += 1;
            h_report->full += full; h_report->partial += !full; h_report->mate2 += second;
            h_report->emptied += cut == a;
        }
    }
    return 0;
}
