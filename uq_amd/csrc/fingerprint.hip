// fingerprint.hip -- the FASTQ record fingerprint `uqfp1`: nine u64 sums over the records of a FASTQ text that say
// whether two texts hold the same reads (in the same order, or as a multiset) and, if not, which line class differs.  An extension: the
// reference has no such check.
//
// The definition (all arithmetic mod 2^64; K = 0x9E3779B97F4A7C15; mix = the splitmix64 finaliser without the increment, synth.hip's
// splitmix64(x) is mix(x + K)):
//   line b[0, L) without its newline, words w_k = little-endian u64 of b[8k, 8k + 8) zero-padded:
//       acc = sum_k mix(w_k + K (k + 1)),   LH(tag, b) = mix(acc + K L + tag)
//   record r (global index) with lines q, s, p, u:  hq = LH(1, q), hs = LH(2, s), hu = LH(4, u),
//       pair = mix(hs + mix(hu)),  rec = mix(hq + pair),  ord = mix(rec + K (r + 1))
//   fingerprint = { reads, bases = sum len(s), plus_text = #records whose line 3 is not exactly "+", sum hq, sum hs, sum hu, sum pair, sum rec, sum ord }
// Every sum commutes, so the result does not depend on how the work is split; calls and shards add.
//
// The kernel reads the stream once and writes nothing but its nine sums (one atomic add per field per workgroup).  Workgroups are persistent
// and walk over groups of G consecutive records, G sized on the device from the shard's average record length so that a typical group is one
// LDS tile.  A group's byte span is staged tile by tile (FP_TILE bytes, cut at 16-byte-aligned addresses, 16-byte coalesced loads); a word
// belongs to the tile that holds its first byte, the staging buffer carries 16 bytes beyond the tile for the words that straddle its end.
// P = 256 / G lanes share a record: the words of its three hashed lines that fall into the tile form one list, lane p takes items p, p + P, ...
// -- a word's term depends on (w_k, k) alone, so a 70 kbp line is simply 8 750 items spread over 256 lanes and nine tiles, never a per-thread
// loop over HBM.  The lanes' partial sums meet in LDS (ds_add_u64) when the group's last tile is done; one lane per record finishes the
// record.  Lines start at any byte: a word is put together from three aligned LDS dwords (v_alignbyte).
// Algorithmic HBM bytes: the record bytes once + 32 B of line offsets per record.
#include "common.h"

namespace {
constexpr int FP_THREADS = 256;
constexpr uint32_t FP_TILE = 16368;                  // bytes of the stream per staged tile (tests/test_gpu_fingerprint.py builds its inputs from this)
constexpr uint32_t FP_NV = FP_TILE / 16 + 1;         // 16-byte vectors staged per tile: the tile + one vector beyond it = four per lane
constexpr uint32_t FP_GMAX = 63;                     // records per group, upper bound: its 4 G + 1 line starts are one per lane, P >= 4 lanes per record
constexpr uint32_t FP_BLOCKS_PER_CU = 5;             // what the kernel's registers admit (__launch_bounds__: 95 VGPRs, 5 waves per SIMD): the persistent grid is one resident round
constexpr uint64_t FP_K = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ uint64_t fp_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// words [klo, khi) of the line at stream offset s with W words start inside the tile [cb, ce)
__device__ __forceinline__ void words_in_tile(int64_t s, uint32_t W, int64_t cb, int64_t ce, uint32_t& klo, uint32_t& khi) {
    klo = 0; khi = 0;
    if (s >= ce) return;
    if (s < cb) { const uint64_t k = (uint64_t)(cb - s + 7) >> 3; klo = k < W ? (uint32_t)k : W; }
    const uint64_t k = (uint64_t)(ce - s + 7) >> 3;
    khi = k < W ? (uint32_t)k : W;
}

__global__ __launch_bounds__(FP_THREADS, FP_BLOCKS_PER_CU) void fingerprint_kernel(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ ls, uint64_t first,
                                                                 uint64_t n, uint64_t index_base, uq_fingerprint* __restrict__ fp) {
    __shared__ __align__(16) uint8_t stage[FP_NV * 16];
    __shared__ uint64_t meta[4 * FP_GMAX + 1];                  // line starts of the group's records (stream offsets)
    __shared__ unsigned long long lacc[3 * FP_GMAX];            // acc of lines 1, 2, 4 of every record of the group
    __shared__ unsigned long long facc[9][FP_GMAX + 1];         // the nine sums, one slot per finishing lane (kept out of the registers the hash loop wants)
    __shared__ uint32_t plusf[FP_GMAX + 1];
    const uint32_t tid = threadIdx.x;
    // the launch geometry is decided here (no device -> host round trip before the launch), the same in every workgroup
    const uint64_t lo = ls[4 * first], hi = ls[4 * (first + n)];                 // the shard's bytes: nothing outside [lo, hi) is loaded
    const uint64_t avg = (hi - lo) / n + 1;
    const uint64_t G64 = (FP_TILE - 64) / (avg + avg / 8 + 1);
    const uint32_t G = (uint32_t)(G64 > FP_GMAX ? FP_GMAX : (G64 < 1 ? 1 : G64));
    const uint32_t P = FP_THREADS / G;                                           // lanes per record, 2 .. 256
    const uint32_t rr = tid / P, pp = tid - rr * P;
    const uint64_t ngroups = (n + G - 1) / G, S = gridDim.x;
    const uint64_t abase = (uint64_t)(uintptr_t)buf;

    // Tiles are cut at 16-byte-aligned ADDRESSES: a group's tile c covers the stream offsets [cb, cb + FP_TILE), cb = t0 + c * FP_TILE, where
    // t0 <= the group's first byte (negative when the buffer itself is misaligned).  The next tile's vectors and, at a group's last tile, the
    // next group's line starts are requested before the current tile is hashed: they stay in registers, in flight, meanwhile.
    struct Regs { uint4 v[FP_NV / FP_THREADS]; uint64_t m; };
    static_assert(4 * FP_GMAX + 1 <= FP_THREADS, "one line start per lane");
    static_assert(FP_NV % FP_THREADS == 0, "whole vectors per lane");
    auto group_t0 = [&](uint64_t gg) { return (int64_t)(((abase + ls[4 * (first + gg * G)]) & ~uint64_t(15)) - abase); };
    auto issue_tile = [&](Regs& x, int64_t cb) {
#pragma unroll
        for (uint32_t u = 0; u < FP_NV / FP_THREADS; ++u) {
            const int64_t o = cb + 16 * (int64_t)(u * FP_THREADS + tid);         // a vector is loaded iff it holds a byte of the shard: it shares that byte's page
            x.v[u] = (o + 16 > (int64_t)lo && o < (int64_t)hi) ? *(const uint4*)(buf + o) : make_uint4(0, 0, 0, 0);
        }
    };
    auto issue_meta = [&](Regs& x, uint64_t gg) {
        const uint64_t r0 = gg * G;
        const uint32_t Rt = (uint32_t)((n - r0) < G ? (n - r0) : G);
        const uint64_t* lsp = ls + 4 * (first + r0);
        x.m = tid <= 4 * Rt ? lsp[tid] : 0;
    };

    if (tid <= FP_GMAX) {
#pragma unroll
        for (int i = 0; i < 9; ++i) facc[i][tid] = 0;
    }
    uint64_t g = blockIdx.x;
    if (g >= ngroups) return;
    Regs cur;
    int64_t t0 = group_t0(g), t0n = g + S < ngroups ? group_t0(g + S) : 0;
    issue_meta(cur, g);
    issue_tile(cur, t0);
    for (; g < ngroups; g += S) {
        const uint64_t r0 = g * G;
        const uint32_t Rt = (uint32_t)((n - r0) < G ? (n - r0) : G);
        const bool more = g + S < ngroups;
        const int64_t t0nn = g + 2 * S < ngroups ? group_t0(g + 2 * S) : 0;      // (a scalar load, asked for two groups ahead: nobody waits for it here)
        if (tid <= 4 * Rt) meta[tid] = cur.m;
        for (uint32_t i = tid; i < 3 * Rt; i += FP_THREADS) lacc[i] = 0;
        uint64_t a0 = 0, a1 = 0, a2 = 0;
        bool plus_ok = false;
        for (int64_t cb = t0;; cb += FP_TILE) {                                   // (a group has at least one tile)
            const int64_t ce = cb + FP_TILE;
            if (cb != t0) __syncthreads();                                        // the previous tile has been read
#pragma unroll
            for (uint32_t u = 0; u < FP_NV / FP_THREADS; ++u) ((uint4*)stage)[u * FP_THREADS + tid] = cur.v[u];
            __syncthreads();
            // the end of the group's span, out of LDS and kept wave-uniform (in SGPRs): a load from HBM here would stall every group's start
            const uint64_t g1v = meta[4 * Rt];
            const int64_t g1 = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(g1v >> 32)) << 32) |
                                          (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)g1v));     // (the builtin returns int: no sign extension)
            const bool last = ce >= g1;
            if (!last) issue_tile(cur, ce);
            else if (more) { issue_meta(cur, g + S); issue_tile(cur, t0n); }
            if (rr < Rt) {
                const int64_t sq = (int64_t)meta[4 * rr], ss = (int64_t)meta[4 * rr + 1], sp = (int64_t)meta[4 * rr + 2], su = (int64_t)meta[4 * rr + 3];
                const uint32_t Lq = (uint32_t)(ss - sq - 1), Ls = (uint32_t)(sp - ss - 1), Lp = (uint32_t)(su - sp - 1),
                               Lu = (uint32_t)((int64_t)meta[4 * rr + 4] - su - 1);
                if (pp == 0 && Lp == 1 && sp >= cb && sp < ce) plus_ok = stage[sp - cb] == '+';
                uint32_t k0, e0, k1, e1, k2, e2;
                words_in_tile(sq, (Lq + 7) >> 3, cb, ce, k0, e0);
                words_in_tile(ss, (Ls + 7) >> 3, cb, ce, k1, e1);
                words_in_tile(su, (Lu + 7) >> 3, cb, ce, k2, e2);
                const uint32_t n0 = e0 - k0, n01 = n0 + (e1 - k1), n012 = n01 + (e2 - k2);       // < 3 * FP_TILE / 8
                // Item i of the record's list is word k = i + dk of its line (dk = the line's first word in the tile - the items in front of it,
                // mod 2^32), so everything an item needs is affine in i: its offset in the tile 8 i + do_ (the line's own offset is negative,
                // mod 2^32, where it began in an earlier tile; the sum lies in [0, FP_TILE)), the bytes its line has left dr - 8 i, and
                // K (k + 1) = K i + dK -- K i is carried along by additions.  Per item only the line's three constants are selected.
                const uint32_t dk0 = k0, dk1 = k1 - n0, dk2 = k2 - n01;
                const uint32_t do0 = (uint32_t)(sq - cb) + 8 * dk0, do1 = (uint32_t)(ss - cb) + 8 * dk1, do2 = (uint32_t)(su - cb) + 8 * dk2;
                const uint32_t dr0 = Lq - 8 * dk0, dr1 = Ls - 8 * dk1, dr2 = Lu - 8 * dk2;
                const uint64_t dK0 = FP_K * (uint64_t)((int64_t)(int32_t)dk0 + 1), dK1 = FP_K * (uint64_t)((int64_t)(int32_t)dk1 + 1),
                               dK2 = FP_K * (uint64_t)((int64_t)(int32_t)dk2 + 1);
                const uint64_t KP = FP_K * (uint64_t)P;
                uint64_t Ki = FP_K * (uint64_t)pp;
                for (uint32_t i = pp; i < n012; i += P, Ki += KP) {
                    const bool in0 = i < n0, in1 = i < n01;
                    const uint32_t o = (in0 ? do0 : (in1 ? do1 : do2)) + 8 * i;   // the word starts inside the tile and ends at most 7 bytes behind it
                    const uint32_t rem = (in0 ? dr0 : (in1 ? dr1 : dr2)) - 8 * i; // bytes of the line from this word on, >= 1: what lies beyond is zero padding
                    const uint64_t dK = in0 ? dK0 : (in1 ? dK1 : dK2);
                    const uint32_t* w = (const uint32_t*)(stage + (o & ~3u));
                    const uint32_t d0 = w[0], d1 = w[1], d2 = w[2];
                    const uint32_t wl = __builtin_amdgcn_alignbyte(d1, d0, o & 3u), wh = __builtin_amdgcn_alignbyte(d2, d1, o & 3u);
                    const uint64_t keep = ~0ull >> (64u - 8u * (rem < 8u ? rem : 8u));
                    const uint64_t t = fp_mix(((((uint64_t)wh << 32) | wl) & keep) + Ki + dK);
                    a0 += in0 ? t : 0; a1 += (!in0 && in1) ? t : 0; a2 += in1 ? 0 : t;
                }
            }
            if (last) break;
        }
        if (rr < Rt) {
            if (a0) atomicAdd(&lacc[3 * rr], (unsigned long long)a0);
            if (a1) atomicAdd(&lacc[3 * rr + 1], (unsigned long long)a1);
            if (a2) atomicAdd(&lacc[3 * rr + 2], (unsigned long long)a2);
            if (pp == 0) plusf[rr] = plus_ok ? 0u : 1u;
        }
        __syncthreads();
        if (tid < Rt) {
            const uint64_t sq = meta[4 * tid], ss = meta[4 * tid + 1], sp = meta[4 * tid + 2], su = meta[4 * tid + 3], e = meta[4 * tid + 4];
            (void)sp;
            const uint64_t Lq = (uint32_t)(ss - sq - 1), Ls = (uint32_t)(sp - ss - 1), Lu = (uint32_t)(e - su - 1);
            const uint64_t hq = fp_mix(lacc[3 * tid] + FP_K * Lq + 1), hs = fp_mix(lacc[3 * tid + 1] + FP_K * Ls + 2),
                           hu = fp_mix(lacc[3 * tid + 2] + FP_K * Lu + 4);
            const uint64_t pair = fp_mix(hs + fp_mix(hu)), rec = fp_mix(hq + pair);
            facc[0][tid] += 1; facc[1][tid] += Ls; facc[2][tid] += plusf[tid]; facc[3][tid] += hq; facc[4][tid] += hs; facc[5][tid] += hu;
            facc[6][tid] += pair; facc[7][tid] += rec; facc[8][tid] += fp_mix(rec + FP_K * (index_base + r0 + tid + 1));
        }
        __syncthreads();                                                          // meta, lacc and the staging buffer are free again
        t0 = t0n; t0n = t0nn;
    }
    // (facc's slots were last written before the loop's closing barrier)
    if (tid < 9 * 16) {
        // field tid / 16: sixteen lanes sum its slots, then one atomic add per field per workgroup
        const uint32_t fld = tid >> 4, l = tid & 15;
        unsigned long long v = 0;
        for (uint32_t i = l; i <= FP_GMAX; i += 16) v += facc[fld][i];
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d, 16);
        if (l == 0 && v) atomicAdd((unsigned long long*)fp + fld, v);
    }
}
}  // namespace

static_assert(sizeof(uq_fingerprint) == 72, "nine u64 fields, no padding");

extern "C" int uq_fingerprint_init(uq_ctx* ctx, uq_fingerprint* d_fp) {
    UQ_REQUIRE(ctx && d_fp, "uq_fingerprint_init: null argument");
    UQ_CHECK_HIP(hipMemsetAsync(d_fp, 0, sizeof(uq_fingerprint), ctx->stream));
    return 0;
}

extern "C" int uq_fingerprint_accumulate(uq_ctx* ctx, const uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                                         uint64_t read_index_base, uq_fingerprint* d_fp) {
    UQ_REQUIRE(ctx && d_buf && d_line_start && d_fp, "uq_fingerprint_accumulate: null argument");
    UQ_REQUIRE(((uintptr_t)d_fp & 7) == 0, "uq_fingerprint_accumulate: d_fp must be 8-byte aligned");
    if (nreads == 0) return 0;
    // the grid needs only an upper bound of the group count (groups hold >= 1 record); surplus workgroups exit at once
    const uint32_t blocks = (uint32_t)(nreads < UQ_NUM_CU * FP_BLOCKS_PER_CU ? nreads : UQ_NUM_CU * FP_BLOCKS_PER_CU);
    fingerprint_kernel<<<blocks, FP_THREADS, 0, ctx->stream>>>(d_buf, d_line_start, first_read, nreads, read_index_base, d_fp);
    UQ_LAUNCH_CHECK();
    return 0;
}

// The sequential twin: the definition as it stands, on host memory; needs no GPU.
extern "C" int uq_fingerprint_host(const uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                                   uint64_t read_index_base, uq_fingerprint* h_fp) {
    UQ_REQUIRE(h_line_start && h_fp && (h_buf || nreads == 0), "uq_fingerprint_host: null argument");
    auto line_hash = [&](uint64_t tag, uint64_t s, uint64_t e) {                 // the line is h_buf[s, e - 1): e = the next line's start
        const uint64_t L = e - s - 1;
        uint64_t acc = 0;
        for (uint64_t k = 0; 8 * k < L; ++k) {
            uint64_t w = 0;
            const uint64_t nb = L - 8 * k < 8 ? L - 8 * k : 8;
            for (uint64_t b = 0; b < nb; ++b) w |= (uint64_t)h_buf[s + 8 * k + b] << (8 * b);
            acc += fp_mix(w + FP_K * (k + 1));
        }
        return fp_mix(acc + FP_K * L + tag);
    };
    for (uint64_t i = 0; i < nreads; ++i) {
        const uint64_t* p = h_line_start + 4 * (first_read + i);
        UQ_REQUIRE(p[0] < p[1] && p[1] < p[2] && p[2] < p[3] && p[3] < p[4], "uq_fingerprint_host: record %llu: line starts out of order",
                   (unsigned long long)(first_read + i));
        const uint64_t hq = line_hash(1, p[0], p[1]), hs = line_hash(2, p[1], p[2]), hu = line_hash(4, p[3], p[4]);
        const uint64_t pair = fp_mix(hs + fp_mix(hu)), rec = fp_mix(hq + pair);
        h_fp->reads += 1; h_fp->bases += p[2] - p[1] - 1;
        h_fp->plus_text += !(p[3] - p[2] == 2 && h_buf[p[2]] == '+');
        h_fp->qname += hq; h_fp->dna += hs; h_fp->qual += hu; h_fp->pairs += pair; h_fp->records += rec;
        h_fp->ordered += fp_mix(rec + FP_K * (read_index_base + i + 1));
    }
    return 0;
}
