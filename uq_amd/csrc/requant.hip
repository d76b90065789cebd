// requant.hip -- `--bin-qual`: a 256-entry byte table applied to every quality line (line 4 of a record, without its newline) of a FASTQ text
// in HBM, in place.  An extension: the reference stores the qualities it is given.
//
// The kernel reads the quality lines and two line starts per record (16 B) and writes the quality lines; the other lines of a record are
// never touched.  Workgroups are persistent and walk over groups of RQ_GROUP consecutive records.  Lane t loads the two line starts of record
// t of the group; the 16-byte-aligned vectors (aligned ADDRESSES: the buffer itself may start anywhere) that hold at least one byte of a
// quality line form one list per group -- a block-wide prefix sum of the vectors per line gives every line its place in it -- and the list is
// worked off in tiles of RQ_TILE bytes: item i of a tile goes to lane i % 256, which finds its line by a binary search over the prefix sums
// in LDS.  So a 70 kbp line is 4 375 items over 256 lanes and five tiles like any other, never a loop of one thread over HBM, and lanes are
// full whatever the mix of lengths.  A lane asks for all RQ_UNROLL vectors of a tile before it touches the first.
//
// Who writes what: an item OWNS the bytes of its vector that belong to its line.  The whole vector is loaded (it holds an owned byte, so it
// lies in the shard's pages; bytes of it that are not owned are not used), and only owned bytes are stored: a vector that is owned whole as
// one 16-byte store, otherwise each wholly owned dword as a dword and the rest byte by byte.  There is no read-modify-write of a byte the item
// does not own, so two lines that share a vector (1-base reads: quality lines a few bytes apart) cannot lose each other's write, and nothing
// outside the lines 4 of [first_read, first_read + nreads) is written.
// The table travels in the kernel arguments and is copied to LDS (256 B: its 64 dwords sit in 64 banks, so a lookup never conflicts).
// Changed bytes are counted per lane, summed per workgroup, one atomic add per workgroup.
#include "common.h"

namespace {
constexpr int RQ_THREADS = 256;
constexpr uint32_t RQ_GROUP = 256;                              // records per group: one lane per record loads its two line starts
constexpr uint32_t RQ_UNROLL = 4;                               // 16-byte vectors a lane has in flight
constexpr uint32_t RQ_TILE = RQ_THREADS * RQ_UNROLL * 16;       // bytes of quality vectors per tile (tests/test_gpu_binqual.py builds its inputs from this)
constexpr uint32_t RQ_BLOCKS_PER_CU = 5;                        // what the kernel's registers admit (86 VGPRs: 5 waves per SIMD; 6 would spill): the persistent grid is one resident round

struct RqLut { uint8_t b[256]; };

__device__ __forceinline__ uint32_t rq_map(const uint8_t* lut, uint32_t x) {
    return (uint32_t)lut[x & 255u] | ((uint32_t)lut[(x >> 8) & 255u] << 8) | ((uint32_t)lut[(x >> 16) & 255u] << 16) | ((uint32_t)lut[x >> 24] << 24);
}

// 0xFF in every byte b of dword d of a vector with lo <= 4 d + b < hi
__device__ __forceinline__ uint32_t rq_own(uint32_t d, uint32_t lo, uint32_t hi) {
    int s = (int)lo - 4 * (int)d, t = (int)hi - 4 * (int)d;
    s = s < 0 ? 0 : (s > 4 ? 4 : s);
    t = t < 0 ? 0 : (t > 4 ? 4 : t);
    if (t <= s) return 0;
    return (uint32_t)((1ull << (8 * t)) - 1) & ~(uint32_t)((1ull << (8 * s)) - 1);
}

__device__ __forceinline__ uint32_t rq_nonzero_bytes(uint32_t x) {
    return __popc((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
}

__global__ __launch_bounds__(RQ_THREADS, RQ_BLOCKS_PER_CU) void requant_kernel(uint8_t* buf, const uint64_t* __restrict__ ls, uint64_t first, uint64_t n,
                                                                                RqLut lut, unsigned long long* changed) {
    __shared__ __align__(16) uint8_t s_lut[256];
    __shared__ uint64_t s_off[RQ_GROUP];                        // vectors of the group's lines in front of line t
    __shared__ uint64_t s_a[RQ_GROUP], s_e[RQ_GROUP];           // ADDRESSES of the first byte of quality line t and of the byte behind its last
    __shared__ uint64_t s_scan[RQ_THREADS / UQ_WAVE + 1];
    __shared__ unsigned long long s_changed;
    const uint32_t tid = threadIdx.x;
    static_assert(RQ_GROUP == RQ_THREADS, "one record per lane");
    if (tid < 64) ((uint32_t*)s_lut)[tid] = ((const uint32_t*)lut.b)[tid];
    if (tid == 0) s_changed = 0;
    const uint64_t abase = (uint64_t)(uintptr_t)buf;
    const uint64_t ngroups = (n + RQ_GROUP - 1) / RQ_GROUP, S = gridDim.x;
    auto load_lines = [&](uint64_t g, uint64_t& a, uint64_t& e) {   // all offsets are 64-bit: nothing here passes through a 32-bit builtin
        const uint64_t r = g * RQ_GROUP + tid;
        a = 0; e = 0;
        if (g < ngroups && r < n) { const uint64_t* p = ls + 4 * (first + r) + 3; a = abase + p[0]; e = abase + p[1] - 1; }
    };
    uint64_t a, e, na, ne;
    uint32_t nchanged = 0;
    load_lines(blockIdx.x, a, e);
    for (uint64_t g = blockIdx.x; g < ngroups; g += S) {
        const uint64_t nv = e > a ? ((e + 15) >> 4) - (a >> 4) : 0;        // an empty line has no vector
        uint64_t total;
        const uint64_t off = block_exclusive_sum<uint64_t, RQ_THREADS / UQ_WAVE>(nv, s_scan, total);
        s_off[tid] = off; s_a[tid] = a; s_e[tid] = e;                     // (lanes beyond the group's records: nv = 0, off = total)
        __syncthreads();
        load_lines(g + S, na, ne);                                         // the next group's line starts are on their way while this one is worked off
        for (uint64_t base = 0; base < total; base += RQ_TILE / 16) {
            uint4 v[RQ_UNROLL];
            int64_t at[RQ_UNROLL];                                         // the vector is at buf + at (never a pointer made of an integer or picked between two: the accesses stay global, not flat)
            uint32_t lohi[RQ_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < RQ_UNROLL; ++u) {
                const uint64_t i = base + u * RQ_THREADS + tid;
                lohi[u] = 0; at[u] = 0; v[u] = make_uint4(0, 0, 0, 0);
                if (i < total) {
                    uint32_t r = 0;                                        // the last line whose first vector is item i or in front of it
#pragma unroll
                    for (uint32_t s = RQ_GROUP / 2; s; s >>= 1) r += s_off[r + s] <= i ? s : 0;
                    const uint64_t la = s_a[r], le = s_e[r];
                    const uint64_t va = (la & ~uint64_t(15)) + 16 * (i - s_off[r]);      // < le: the vector holds a byte of the line
                    const uint32_t lo = va < la ? (uint32_t)(la - va) : 0u;
                    const uint32_t hi = le - va < 16 ? (uint32_t)(le - va) : 16u;
                    at[u] = (int64_t)(va - abase);                         // (negative for a first vector that begins in front of a misaligned buffer)
                    lohi[u] = lo | (hi << 8);                              // hi >= 1: non-zero for every item
                    v[u] = *(const uint4*)(buf + at[u]);
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < RQ_UNROLL; ++u) {
                if (!lohi[u]) continue;
                const uint32_t lo = lohi[u] & 255u, hi = lohi[u] >> 8;
                uint8_t* const p = buf + at[u];
                const uint32_t x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                uint32_t y[4];
#pragma unroll
                for (uint32_t d = 0; d < 4; ++d) y[d] = rq_map(s_lut, x[d]);
                if (lo == 0 && hi == 16) {
#pragma unroll
                    for (uint32_t d = 0; d < 4; ++d) nchanged += rq_nonzero_bytes(x[d] ^ y[d]);
                    *(uint4*)p = make_uint4(y[0], y[1], y[2], y[3]);
                } else {
#pragma unroll
                    for (uint32_t d = 0; d < 4; ++d) {
                        const uint32_t m = rq_own(d, lo, hi);
                        nchanged += rq_nonzero_bytes((x[d] ^ y[d]) & m);
                        if (m == ~0u) ((uint32_t*)p)[d] = y[d];
                        else if (m) {
#pragma unroll
                            for (uint32_t b = 0; b < 4; ++b)
                                if ((m >> (8 * b)) & 1u) p[4 * d + b] = (uint8_t)(y[d] >> (8 * b));
                        }
                    }
                }
            }
        }
        __syncthreads();                                                   // s_off, s_a, s_e are free again
        a = na; e = ne;
    }
    if (changed) {
        const uint32_t w = wave_sum(nchanged);                             // < 2^32: a lane changes at most 16 bytes per item
        if (lane_id() == 0 && w) atomicAdd(&s_changed, (unsigned long long)w);
        __syncthreads();
        if (tid == 0 && s_changed) atomicAdd(changed, s_changed);
    }
}

int rq_check_lut(const uint8_t* h_lut, const char* who) {
    // (lut['\n'] itself is never applied -- a line holds no newline -- so the identity's '\n' -> '\n' passes)
    for (int i = 0; i < 256; ++i) UQ_REQUIRE(i == '\n' || h_lut[i] != '\n', "%s: lut[%d] is a newline: the table must not make line ends", who, i);
    return 0;
}
}  // namespace

extern "C" int uq_requantise_qualities(uq_ctx* ctx, uint8_t* d_buf, const uint64_t* d_line_start, uint64_t first_read, uint64_t nreads,
                                       const uint8_t* h_lut, uint64_t* d_changed) {
    UQ_REQUIRE(ctx && d_line_start && h_lut && (d_buf || nreads == 0), "uq_requantise_qualities: null argument");
    UQ_REQUIRE(((uintptr_t)d_changed & 7) == 0, "uq_requantise_qualities: d_changed must be 8-byte aligned");
    UQ_TRY(rq_check_lut(h_lut, "uq_requantise_qualities"));
    if (nreads == 0) return 0;
    RqLut lut;
    memcpy(lut.b, h_lut, 256);
    const uint64_t ngroups = (nreads + RQ_GROUP - 1) / RQ_GROUP;
    const uint32_t blocks = (uint32_t)(ngroups < UQ_NUM_CU * RQ_BLOCKS_PER_CU ? ngroups : UQ_NUM_CU * RQ_BLOCKS_PER_CU);
    requant_kernel<<<blocks, RQ_THREADS, 0, ctx->stream>>>(d_buf, d_line_start, first_read, nreads, lut, (unsigned long long*)d_changed);
    UQ_LAUNCH_CHECK();
    return 0;
}

// The sequential twin: the definition as it stands, on host memory; needs no GPU.
extern "C" int uq_requantise_qualities_host(uint8_t* h_buf, const uint64_t* h_line_start, uint64_t first_read, uint64_t nreads,
                                            const uint8_t* h_lut, uint64_t* h_changed) {
    UQ_REQUIRE(h_line_start && h_lut && (h_buf || nreads == 0), "uq_requantise_qualities_host: null argument");
    UQ_TRY(rq_check_lut(h_lut, "uq_requantise_qualities_host"));
    uint64_t changed = 0;
    for (uint64_t i = 0; i < nreads; ++i) {
        const uint64_t* p = h_line_start + 4 * (first_read + i);
        UQ_REQUIRE(p[3] < p[4], "uq_requantise_qualities_host: record %llu: line starts out of order", (unsigned long long)(first_read + i));
        for (uint64_t k = p[3]; k + 1 < p[4]; ++k) {
            const uint8_t y = h_lut[h_buf[k]];
            changed += y != h_buf[k];
            h_buf[k] = y;
        }
    }
    if (h_changed) *h_changed += changed;
    return 0;
}
