// deflate.hip -- BGZF output: a device buffer compressed into a BGZF stream (uq_bgzf_compress: one workgroup per 65 280-byte block), and
// the host run of the same compressor on one block (uq_bgzf_compress_block_host).
//
// The compressor is deflate_core.h.  Here it gets its two environments:
//   device  the block in LDS (16-byte loads), the per-position distances in an HBM workspace (65 280 u16 per block), the member written
//           into a zeroed 64 KiB slot of HBM (whole words stored, the words shared by two bit ranges OR-ed with global atomics);
//   host    plain arrays, one "thread".
// uq_bgzf_compress works through the blocks in chunks: compress every block of the chunk into its slot, scan the sizes, copy the members
// into place at their 64-bit offsets; the workspace is bounded by the chunk, not by the stream.  uq_bgzf_compress_parts does the same over
// a list of buffers, each behind a short host prefix (a tar member's .npy header): one block table for all of them, the chunks running
// across the buffers, the block cuts restarting at every buffer.
//
// LDS: UqDeflateLds is about 151 KiB (the block, one match-length byte per position, the head table / parse window / Huffman scratch, the
// code tables): one workgroup of UQ_DEF_THREADS threads per CU.  Level 2 (UQ_BGZF_LEVEL2: UqDeflateLds2) adds 1 KiB; the workspace and
// everything around the compressor are the same for both levels.
#include "inflate_env.h"
#include "deflate_core.h"
#include <vector>

#define UQ_DEF_THREADS 512
#define UQ_DEF_CHUNK 2048u                   // blocks per pass: 2048 x (64 KiB slot + 127.5 KiB distances) = 383 MiB of workspace
#define UQ_DEF_SLOT 65536u

namespace {

struct DevEnv {
    uint32_t* out;              // the block's slot
    uint16_t* dist;             // the block's distance workspace
    const uint32_t* x2n;        // LDS
    __device__ void sync() { __syncthreads(); }
    __device__ void lds_max(uint32_t* p, uint32_t v) { atomicMax(p, v); }
    __device__ void lds_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
    __device__ void lds_xor(uint32_t* p, uint32_t v) { atomicXor(p, v); }
    __device__ void dist_put(uint32_t p, uint32_t d) { dist[p] = (uint16_t)d; }
    __device__ uint32_t dist_get(uint32_t p) const { return dist[p]; }
    __device__ void word_store(uint32_t w, uint32_t v) { out[w] = v; }
    __device__ void word_or(uint32_t w, uint32_t v) { atomicOr(out + w, v); }
};

template <int kLevel> struct LdsOf { typedef UqDeflateLds type; };
template <> struct LdsOf<2> { typedef UqDeflateLds2 type; };

template <int kLevel>
__global__ __launch_bounds__(UQ_DEF_THREADS) void bgzf_deflate_kernel(const uint8_t* __restrict__ in, uint64_t nbytes, uint64_t first_block,
                                                                      uint8_t* __restrict__ slots, uint16_t* __restrict__ dist,
                                                                      uint32_t* __restrict__ sizes, uint32_t* __restrict__ status, X2n x2n) {
    __shared__ __attribute__((aligned(16))) typename LdsOf<kLevel>::type s;
    __shared__ uint32_t x2n_s[32];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const uint64_t off = (first_block + b) * (uint64_t)UQ_DEF_MAX_IN;
    const uint32_t n = (uint32_t)(nbytes - off < UQ_DEF_MAX_IN ? nbytes - off : UQ_DEF_MAX_IN);
    if (tid < 32) x2n_s[tid] = x2n.v[tid];
    const uint8_t* src = in + off;
    uint32_t i0 = 0;
    if (((uintptr_t)src & 15) == 0) {
        const uint32_t nv = n / 16;
        for (uint32_t v = tid; v < nv; v += UQ_DEF_THREADS) ((uint4*)s.in)[v] = ((const uint4*)src)[v];
        i0 = nv * 16;
    }
    for (uint32_t i = i0 + tid; i < n; i += UQ_DEF_THREADS) s.in[i] = src[i];
    __syncthreads();
    DevEnv env{(uint32_t*)(slots + (uint64_t)b * UQ_DEF_SLOT), dist + (uint64_t)b * UQ_DEF_MAX_IN, x2n_s};
    uint32_t mb = 0;
    const int st = uq_deflate_block_l<kLevel>(env, &s, n, UQ_DEF_SLOT, tid, UQ_DEF_THREADS, &mb);
    if (tid == 0) { sizes[b] = st == UQ_DEF_OK ? mb : 0; status[b] = (uint32_t)st; }
}

// member b of the chunk: slot b[0, sizes[b]) -> out[base + offs[b], ...); the output words that lie inside the member are written whole,
// the bytes at its two ends one by one (they share a word with the neighbouring members)
__global__ __launch_bounds__(256) void bgzf_place_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes,
                                                         const uint32_t* __restrict__ offs, uint8_t* __restrict__ out, uint64_t base) {
    const uint32_t b = blockIdx.x, tid = threadIdx.x, n = sizes[b];
    const uint32_t* src = (const uint32_t*)(slots + (uint64_t)b * UQ_DEF_SLOT);
    const uint8_t* s8 = (const uint8_t*)src;
    uint8_t* dst = out + base + offs[b];
    const uint32_t lead = (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3), head = lead < n ? lead : n;
    const uint32_t nw = (n - head) / 4, sh = head * 8;
    if (tid < head) dst[tid] = s8[tid];
    uint32_t* dw = (uint32_t*)(dst + head);
    for (uint32_t w = tid; w < nw; w += 256) {
        // member bytes [head + 4w, head + 4w + 4): inside slot words w and w + 1 (n <= 65 311: w + 1 stays inside the 64 KiB slot)
        const uint32_t lo = src[w], hi = src[w + 1];
        dw[w] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    }
    for (uint32_t i = head + 4 * nw + tid; i < n; i += 256) dst[i] = s8[i];
}

// ---- uq_bgzf_compress_parts: several buffers, each behind a short host prefix, as one run of members.  One table entry per block:
struct PartBlock { uint64_t off; uint32_t part; uint32_t n; };      // bytes [off, off + n) of prefix || data of `part`
struct PartSrc { const uint8_t* data; uint32_t prefix_bytes; uint32_t reserved; };

#define UQ_PARTS_MAX_PREFIX 256u

typedef const __attribute__((address_space(1))) uint8_t* GlobalBytes;
typedef uint32_t Vec4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) Vec4* GlobalVecs;

// dwords [WS, WS + 4] of a || c, shifted right by r bits (r = 0, 8, 16 or 24) into four dwords
template <int WS> __device__ __forceinline__ Vec4 shifted_vec(Vec4 a, Vec4 c, uint32_t r) {
    const uint32_t d[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
    Vec4 o;
    o.x = r ? (d[WS] >> r) | (d[WS + 1] << (32 - r)) : d[WS];
    o.y = r ? (d[WS + 1] >> r) | (d[WS + 2] << (32 - r)) : d[WS + 1];
    o.z = r ? (d[WS + 2] >> r) | (d[WS + 3] << (32 - r)) : d[WS + 2];
    o.w = r ? (d[WS + 3] >> r) | (d[WS + 4] << (32 - r)) : d[WS + 3];
    return o;
}

// The block of table entry first_block + blockIdx.x into LDS, then the compressor.  in[0, lo) comes from the part's prefix in the arena
// (block 0 of a part only: a prefix is at most 256 bytes), in[lo, n) from the part's buffer.  The LDS side is written in whole 16-byte
// vectors whatever the source's alignment: a source that is not 16-byte aligned is read as the two aligned 16-byte vectors that cover
// the wanted one (each holds at least one byte of it, so no read leaves the buffer's 16-byte granules) and shifted into place.
template <int kLevel>
__global__ __launch_bounds__(UQ_DEF_THREADS) void bgzf_deflate_parts_kernel(const PartBlock* __restrict__ table, const PartSrc* __restrict__ parts,
                                                                            const uint8_t* __restrict__ arena, uint64_t first_block,
                                                                            uint8_t* __restrict__ slots, uint16_t* __restrict__ dist,
                                                                            uint32_t* __restrict__ sizes, uint32_t* __restrict__ status, X2n x2n) {
    __shared__ __attribute__((aligned(16))) typename LdsOf<kLevel>::type s;
    __shared__ uint32_t x2n_s[32];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const PartBlock e = table[first_block + b];
    const PartSrc ps = parts[e.part];
    const uint32_t n = e.n < UQ_DEF_MAX_IN ? e.n : UQ_DEF_MAX_IN;
    if (tid < 32) x2n_s[tid] = x2n.v[tid];
    const uint32_t lo = e.off < ps.prefix_bytes ? ((uint32_t)(ps.prefix_bytes - e.off) < n ? (uint32_t)(ps.prefix_bytes - e.off) : n) : 0;
    if (tid < lo) s.in[tid] = arena[(uint64_t)e.part * UQ_PARTS_MAX_PREFIX + e.off + tid];
    // src[i] = byte i of the block, for i >= lo; the pointer comes out of a table, so the compiler is told that it is global memory
    const GlobalBytes src = (GlobalBytes)(ps.data + ((ptrdiff_t)e.off - (ptrdiff_t)ps.prefix_bytes));
    const uint32_t v0 = (lo + 15) / 16, v1 = n / 16;                              // whole vectors of in[lo, n): [v0, v1)
    const uint32_t head_end = v0 * 16 < n ? v0 * 16 : n;
    for (uint32_t i = lo + tid; i < head_end; i += UQ_DEF_THREADS) s.in[i] = src[i];
    uint32_t tail = head_end;
    if (v1 > v0) {
        const uint32_t mis = (uint32_t)((uintptr_t)src & 15);
        if (mis == 0) {
            for (uint32_t v = v0 + tid; v < v1; v += UQ_DEF_THREADS) ((Vec4*)s.in)[v] = ((GlobalVecs)src)[v];
        } else {
            // vector v of the block = bytes [mis, mis + 16) of the aligned vectors v and v + 1 behind src - mis: two 16-byte loads in
            // flight, then the shift (the same for the whole workgroup)
            const GlobalVecs q = (GlobalVecs)(src - mis);
            const uint32_t r = (mis & 3) * 8;
            for (uint32_t v = v0 + tid; v < v1; v += UQ_DEF_THREADS) {
                const Vec4 a = q[v], c = q[v + 1];
                switch (mis >> 2) {
                    case 0: ((Vec4*)s.in)[v] = shifted_vec<0>(a, c, r); break;
                    case 1: ((Vec4*)s.in)[v] = shifted_vec<1>(a, c, r); break;
                    case 2: ((Vec4*)s.in)[v] = shifted_vec<2>(a, c, r); break;
                    default: ((Vec4*)s.in)[v] = shifted_vec<3>(a, c, r); break;
                }
            }
        }
        tail = v1 * 16;
    }
    for (uint32_t i = tail + tid; i < n; i += UQ_DEF_THREADS) s.in[i] = src[i];
    __syncthreads();
    DevEnv env{(uint32_t*)(slots + (uint64_t)b * UQ_DEF_SLOT), dist + (uint64_t)b * UQ_DEF_MAX_IN, x2n_s};
    uint32_t mb = 0;
    const int st = e.n > UQ_DEF_MAX_IN ? (int)UQ_DEF_TOO_LARGE : uq_deflate_block_l<kLevel>(env, &s, n, UQ_DEF_SLOT, tid, UQ_DEF_THREADS, &mb);
    if (tid == 0) { sizes[b] = st == UQ_DEF_OK ? mb : 0; status[b] = (uint32_t)st; }
}

// the chunk's scan gives every part's bytes in the chunk: (end of its last block) - (start of its first block), added to part_bytes
__global__ void bgzf_part_totals_kernel(const PartBlock* __restrict__ table, uint64_t first_block, uint32_t nb, const uint32_t* __restrict__ sizes,
                                        const uint32_t* __restrict__ offs, unsigned long long* __restrict__ part_bytes) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const uint32_t part = table[first_block + b].part;
    if (b == 0 || table[first_block + b - 1].part != part) atomicAdd(part_bytes + part, 0ull - (unsigned long long)offs[b]);
    if (b == nb - 1 || table[first_block + b + 1].part != part) atomicAdd(part_bytes + part, (unsigned long long)offs[b] + sizes[b]);
}

struct HostEnv {
    uint8_t* out;
    uint32_t limit;             // bytes of `out` that may be written
    uint16_t* dist;
    const uint32_t* x2n;
    void sync() {}
    void lds_max(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
    void lds_add(uint32_t* p, uint32_t v) { *p += v; }
    void lds_xor(uint32_t* p, uint32_t v) { *p ^= v; }
    void dist_put(uint32_t p, uint32_t d) { dist[p] = (uint16_t)d; }
    uint32_t dist_get(uint32_t p) const { return dist[p]; }
    void word_store(uint32_t w, uint32_t v) {
        for (uint32_t k = 0; k < 4; ++k)
            if ((uint64_t)4 * w + k < limit) out[4 * w + k] = (uint8_t)(v >> (8 * k));
    }
    void word_or(uint32_t w, uint32_t v) {
        for (uint32_t k = 0; k < 4; ++k)
            if ((uint64_t)4 * w + k < limit) out[4 * w + k] |= (uint8_t)(v >> (8 * k));
    }
};

const uint8_t BGZF_EOF[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

}  // namespace

extern "C" int uq_bgzf_bound(uint64_t nbytes, uint64_t* h_bound) {
    UQ_REQUIRE(h_bound, "uq_bgzf_bound: null argument");
    *h_bound = (nbytes + UQ_DEF_MAX_IN - 1) / UQ_DEF_MAX_IN * (uint64_t)UQ_DEF_MAX_MEMBER + sizeof(BGZF_EOF);
    return 0;
}

extern "C" int uq_bgzf_compress(uq_ctx* c, const uint8_t* d_in, uint64_t nbytes, uint8_t* d_out, uint64_t out_capacity, uint64_t* h_out_bytes,
                                uint32_t flags) {
    UQ_REQUIRE(c && h_out_bytes, "uq_bgzf_compress: null argument");
    UQ_REQUIRE((d_in || !nbytes) && (d_out || !out_capacity), "uq_bgzf_compress: null buffer");
    UQ_REQUIRE(!(flags & ~(uint32_t)(UQ_BGZF_EOF | UQ_BGZF_LEVEL2)), "uq_bgzf_compress: unknown flags 0x%x", flags);
    *h_out_bytes = 0;
    const uint64_t nblocks = (nbytes + UQ_DEF_MAX_IN - 1) / UQ_DEF_MAX_IN;
    const uint32_t chunk = (uint32_t)(nblocks < UQ_DEF_CHUNK ? nblocks : UQ_DEF_CHUNK);
    uint64_t base = 0;
    if (chunk) {
        ScratchPlan plan;
        const size_t o_slots = plan.add((size_t)chunk * UQ_DEF_SLOT), o_dist = plan.add((size_t)chunk * UQ_DEF_MAX_IN * 2);
        const size_t o_sizes = plan.add(chunk * 4), o_offs = plan.add(chunk * 4), o_status = plan.add(chunk * 4), o_total = plan.add(8);
        void* ws;
        UQ_TRY(uq_scratch(c, plan.off, &ws));
        uint8_t* w8 = (uint8_t*)ws;
        uint8_t* slots = w8 + o_slots;
        uint16_t* dist = (uint16_t*)(w8 + o_dist);
        uint32_t* sizes = (uint32_t*)(w8 + o_sizes);
        uint32_t* offs = (uint32_t*)(w8 + o_offs);
        uint32_t* status = (uint32_t*)(w8 + o_status);
        uint64_t* total = (uint64_t*)(w8 + o_total);
        X2n x2n;
        uq_crc_x2n_init(x2n.v);
        uint32_t* h_status = new uint32_t[chunk];
        for (uint64_t b0 = 0; b0 < nblocks; b0 += chunk) {
            const uint32_t nb = (uint32_t)(nblocks - b0 < chunk ? nblocks - b0 : chunk);
            hipError_t e = hipMemsetAsync(slots, 0, (size_t)nb * UQ_DEF_SLOT, c->stream);
            if (e == hipSuccess) {
                if (flags & UQ_BGZF_LEVEL2) bgzf_deflate_kernel<2><<<nb, UQ_DEF_THREADS, 0, c->stream>>>(d_in, nbytes, b0, slots, dist, sizes, status, x2n);
                else bgzf_deflate_kernel<1><<<nb, UQ_DEF_THREADS, 0, c->stream>>>(d_in, nbytes, b0, slots, dist, sizes, status, x2n);
                e = hipGetLastError();
            }
            const int r = e == hipSuccess ? uq_scan_exclusive_u32(c, sizes, offs, nb, total) : 0;
            uint64_t h_total = 0;
            if (e == hipSuccess && !r) e = hipMemcpyAsync(h_status, status, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess && !r) e = hipMemcpyAsync(&h_total, total, 8, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess && !r) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess || r) {
                delete[] h_status;
                UQ_CHECK_HIP(e);
                return r;
            }
            uint32_t bad = nb;
            for (uint32_t k = 0; k < nb && bad == nb; ++k)
                if (h_status[k]) bad = k;
            const uint32_t bad_status = bad < nb ? h_status[bad] : 0;
            if (bad < nb || base + h_total > out_capacity) delete[] h_status;
            UQ_REQUIRE(bad == nb, "uq_bgzf_compress: block %llu (input bytes from %llu) failed with status %u", (unsigned long long)(b0 + bad),
                       (unsigned long long)((b0 + bad) * UQ_DEF_MAX_IN), bad_status);
            UQ_REQUIRE(base + h_total <= out_capacity, "uq_bgzf_compress: output capacity %llu bytes is too small (uq_bgzf_bound gives the "
                       "capacity needed)", (unsigned long long)out_capacity);
            bgzf_place_kernel<<<nb, 256, 0, c->stream>>>(slots, sizes, offs, d_out, base);
            e = hipGetLastError();
            if (e != hipSuccess) delete[] h_status;
            UQ_CHECK_HIP(e);
            base += h_total;
        }
        delete[] h_status;
    }
    if (flags & UQ_BGZF_EOF) {
        UQ_REQUIRE(base + sizeof(BGZF_EOF) <= out_capacity, "uq_bgzf_compress: output capacity %llu bytes is too small for the EOF member",
                   (unsigned long long)out_capacity);
        UQ_CHECK_HIP(hipMemcpyAsync(d_out + base, BGZF_EOF, sizeof(BGZF_EOF), hipMemcpyHostToDevice, c->stream));
        base += sizeof(BGZF_EOF);
    }
    UQ_CHECK_HIP(hipStreamSynchronize(c->stream));
    *h_out_bytes = base;
    return 0;
}

static int parts_check(const uq_bgzf_part* h_parts, uint32_t nparts, const char* who, uint64_t* nblocks) {
    UQ_REQUIRE(h_parts || !nparts, "%s: null argument", who);
    uint64_t nb = 0;
    for (uint32_t k = 0; k < nparts; ++k) {
        const uq_bgzf_part& p = h_parts[k];
        UQ_REQUIRE(p.prefix_bytes <= UQ_PARTS_MAX_PREFIX, "%s: part %u: a prefix of %u bytes (at most %u)", who, k, p.prefix_bytes, UQ_PARTS_MAX_PREFIX);
        UQ_REQUIRE(p.nbytes <= (UINT64_MAX >> 2), "%s: part %u: nbytes out of range", who, k);
        UQ_REQUIRE((p.h_prefix || !p.prefix_bytes) && (p.d_data || !p.nbytes), "%s: part %u: null buffer", who, k);
        nb += (p.prefix_bytes + p.nbytes + UQ_DEF_MAX_IN - 1) / UQ_DEF_MAX_IN;
        UQ_REQUIRE(nb <= (UINT64_MAX >> 20), "%s: too many blocks", who);
    }
    *nblocks = nb;
    return 0;
}

extern "C" int uq_bgzf_parts_bound(const uq_bgzf_part* h_parts, uint32_t nparts, uint64_t* h_bound) {
    UQ_REQUIRE(h_bound, "uq_bgzf_parts_bound: null argument");
    uint64_t nblocks = 0;
    UQ_TRY(parts_check(h_parts, nparts, "uq_bgzf_parts_bound", &nblocks));
    *h_bound = nblocks * (uint64_t)UQ_DEF_MAX_MEMBER + sizeof(BGZF_EOF);
    return 0;
}

extern "C" int uq_bgzf_compress_parts(uq_ctx* c, const uq_bgzf_part* h_parts, uint32_t nparts, uint8_t* d_out, uint64_t out_capacity,
                                      uint64_t* h_part_bytes, uint64_t* h_out_bytes, uint32_t flags) {
    UQ_REQUIRE(c && h_out_bytes && (h_part_bytes || !nparts), "uq_bgzf_compress_parts: null argument");
    UQ_REQUIRE(d_out || !out_capacity, "uq_bgzf_compress_parts: null buffer");
    UQ_REQUIRE(!(flags & ~(uint32_t)(UQ_BGZF_EOF | UQ_BGZF_LEVEL2)), "uq_bgzf_compress_parts: unknown flags 0x%x", flags);
    *h_out_bytes = 0;
    uint64_t nblocks = 0;
    UQ_TRY(parts_check(h_parts, nparts, "uq_bgzf_compress_parts", &nblocks));
    for (uint32_t k = 0; k < nparts; ++k) h_part_bytes[k] = 0;
    const uint32_t chunk = (uint32_t)(nblocks < UQ_DEF_CHUNK ? nblocks : UQ_DEF_CHUNK);
    uint64_t base = 0;
    if (chunk) {
        // the block table, the parts and their prefixes: built here, uploaded once
        std::vector<PartBlock> h_table((size_t)nblocks);
        std::vector<PartSrc> h_src(nparts);
        std::vector<uint8_t> h_arena((size_t)nparts * UQ_PARTS_MAX_PREFIX, 0);
        uint64_t g = 0;
        for (uint32_t k = 0; k < nparts; ++k) {
            const uq_bgzf_part& p = h_parts[k];
            h_src[k] = PartSrc{p.d_data, p.prefix_bytes, 0};
            if (p.prefix_bytes) memcpy(h_arena.data() + (size_t)k * UQ_PARTS_MAX_PREFIX, p.h_prefix, p.prefix_bytes);
            const uint64_t all = p.prefix_bytes + p.nbytes;
            for (uint64_t off = 0; off < all; off += UQ_DEF_MAX_IN)
                h_table[g++] = PartBlock{off, k, (uint32_t)(all - off < UQ_DEF_MAX_IN ? all - off : UQ_DEF_MAX_IN)};
        }
        ScratchPlan plan;
        const size_t o_slots = plan.add((size_t)chunk * UQ_DEF_SLOT), o_dist = plan.add((size_t)chunk * UQ_DEF_MAX_IN * 2);
        const size_t o_sizes = plan.add(chunk * 4), o_offs = plan.add(chunk * 4), o_status = plan.add(chunk * 4), o_total = plan.add(8);
        const size_t o_table = plan.add(h_table.size() * sizeof(PartBlock)), o_src = plan.add(h_src.size() * sizeof(PartSrc));
        const size_t o_arena = plan.add(h_arena.size()), o_pbytes = plan.add((size_t)nparts * 8);
        void* ws;
        UQ_TRY(uq_scratch(c, plan.off, &ws));
        uint8_t* w8 = (uint8_t*)ws;
        uint8_t* slots = w8 + o_slots;
        uint16_t* dist = (uint16_t*)(w8 + o_dist);
        uint32_t* sizes = (uint32_t*)(w8 + o_sizes);
        uint32_t* offs = (uint32_t*)(w8 + o_offs);
        uint32_t* status = (uint32_t*)(w8 + o_status);
        uint64_t* total = (uint64_t*)(w8 + o_total);
        PartBlock* table = (PartBlock*)(w8 + o_table);
        PartSrc* src = (PartSrc*)(w8 + o_src);
        uint8_t* arena = w8 + o_arena;
        unsigned long long* pbytes = (unsigned long long*)(w8 + o_pbytes);
        UQ_CHECK_HIP(hipMemcpyAsync(table, h_table.data(), h_table.size() * sizeof(PartBlock), hipMemcpyHostToDevice, c->stream));
        UQ_CHECK_HIP(hipMemcpyAsync(src, h_src.data(), h_src.size() * sizeof(PartSrc), hipMemcpyHostToDevice, c->stream));
        UQ_CHECK_HIP(hipMemcpyAsync(arena, h_arena.data(), h_arena.size(), hipMemcpyHostToDevice, c->stream));
        UQ_CHECK_HIP(hipMemsetAsync(pbytes, 0, (size_t)nparts * 8, c->stream));
        X2n x2n;
        uq_crc_x2n_init(x2n.v);
        std::vector<uint32_t> h_status(chunk);
        for (uint64_t b0 = 0; b0 < nblocks; b0 += chunk) {
            const uint32_t nb = (uint32_t)(nblocks - b0 < chunk ? nblocks - b0 : chunk);
            UQ_CHECK_HIP(hipMemsetAsync(slots, 0, (size_t)nb * UQ_DEF_SLOT, c->stream));
            if (flags & UQ_BGZF_LEVEL2)
                bgzf_deflate_parts_kernel<2><<<nb, UQ_DEF_THREADS, 0, c->stream>>>(table, src, arena, b0, slots, dist, sizes, status, x2n);
            else bgzf_deflate_parts_kernel<1><<<nb, UQ_DEF_THREADS, 0, c->stream>>>(table, src, arena, b0, slots, dist, sizes, status, x2n);
            UQ_LAUNCH_CHECK();
            UQ_TRY(uq_scan_exclusive_u32(c, sizes, offs, nb, total));
            uint64_t h_total = 0;
            UQ_CHECK_HIP(hipMemcpyAsync(h_status.data(), status, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
            UQ_CHECK_HIP(hipMemcpyAsync(&h_total, total, 8, hipMemcpyDeviceToHost, c->stream));
            UQ_CHECK_HIP(hipStreamSynchronize(c->stream));
            for (uint32_t k = 0; k < nb; ++k) {
                const PartBlock& e = h_table[(size_t)(b0 + k)];
                UQ_REQUIRE(!h_status[k], "uq_bgzf_compress_parts: part %u, block %llu (bytes of the part from %llu) failed with status %u", e.part,
                           (unsigned long long)(e.off / UQ_DEF_MAX_IN), (unsigned long long)e.off, h_status[k]);
            }
            UQ_REQUIRE(base + h_total <= out_capacity, "uq_bgzf_compress_parts: output capacity %llu bytes is too small (uq_bgzf_parts_bound gives "
                       "the capacity needed)", (unsigned long long)out_capacity);
            bgzf_part_totals_kernel<<<(nb + 255) / 256, 256, 0, c->stream>>>(table, b0, nb, sizes, offs, pbytes);
            UQ_LAUNCH_CHECK();
            bgzf_place_kernel<<<nb, 256, 0, c->stream>>>(slots, sizes, offs, d_out, base);
            UQ_LAUNCH_CHECK();
            base += h_total;
        }
        UQ_CHECK_HIP(hipMemcpyAsync(h_part_bytes, pbytes, (size_t)nparts * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (flags & UQ_BGZF_EOF) {
        UQ_REQUIRE(base + sizeof(BGZF_EOF) <= out_capacity, "uq_bgzf_compress_parts: output capacity %llu bytes is too small for the EOF member",
                   (unsigned long long)out_capacity);
        UQ_CHECK_HIP(hipMemcpyAsync(d_out + base, BGZF_EOF, sizeof(BGZF_EOF), hipMemcpyHostToDevice, c->stream));
        base += sizeof(BGZF_EOF);
    }
    UQ_CHECK_HIP(hipStreamSynchronize(c->stream));
    *h_out_bytes = base;
    return 0;
}

template <int kLevel>
static int block_host(const uint8_t* h_in, uint64_t nbytes, uint8_t* h_out, uint64_t capacity, uint64_t* h_out_bytes, uint32_t* h_status) {
    *h_out_bytes = 0;
    if (nbytes > UQ_DEF_MAX_IN) { *h_status = UQ_DEF_TOO_LARGE; return 0; }
    typename LdsOf<kLevel>::type* s = new typename LdsOf<kLevel>::type();
    uint16_t* dist = new uint16_t[UQ_DEF_MAX_IN];
    uint32_t x2n[32];
    uq_crc_x2n_init(x2n);
    if (nbytes) memcpy(s->in, h_in, nbytes);
    const uint32_t cap = (uint32_t)(capacity < UQ_DEF_SLOT ? capacity : UQ_DEF_SLOT);
    if (cap) memset(h_out, 0, cap);
    HostEnv env{h_out, cap, dist, x2n};
    uint32_t mb = 0;
    const int st = uq_deflate_block_l<kLevel>(env, s, (uint32_t)nbytes, cap, 0, 1, &mb);
    delete[] dist;
    delete s;
    *h_status = (uint32_t)st;
    *h_out_bytes = mb;
    return 0;
}

extern "C" int uq_bgzf_compress_block_host(const uint8_t* h_in, uint64_t nbytes, uint8_t* h_out, uint64_t capacity, uint64_t* h_out_bytes,
                                           uint32_t* h_status) {
    UQ_REQUIRE(h_out_bytes && h_status && (h_in || !nbytes) && (h_out || !capacity), "uq_bgzf_compress_block_host: null argument");
    return block_host<1>(h_in, nbytes, h_out, capacity, h_out_bytes, h_status);
}

extern "C" int uq_bgzf_compress_block_host_l(const uint8_t* h_in, uint64_t nbytes, uint8_t* h_out, uint64_t capacity, uint64_t* h_out_bytes,
                                             uint32_t* h_status, uint32_t flags) {
    UQ_REQUIRE(h_out_bytes && h_status && (h_in || !nbytes) && (h_out || !capacity), "uq_bgzf_compress_block_host_l: null argument");
    UQ_REQUIRE(!(flags & ~(uint32_t)UQ_BGZF_LEVEL2), "uq_bgzf_compress_block_host_l: unknown flags 0x%x", flags);
    return flags & UQ_BGZF_LEVEL2 ? block_host<2>(h_in, nbytes, h_out, capacity, h_out_bytes, h_status)
                                  : block_host<1>(h_in, nbytes, h_out, capacity, h_out_bytes, h_status);
}
