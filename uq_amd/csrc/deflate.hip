// deflate.hip -- BGZF output: a device buffer compressed into a BGZF stream (uq_bgzf_compress: one workgroup per 65 280-byte block), and
// the host run of the same compressor on one block (uq_bgzf_compress_block_host).
//
// The compressor is deflate_core.h.  Here it gets its two environments:
//   device  the block in LDS (16-byte loads), the per-position distances in an HBM workspace (65 280 u16 per block), the member written
//           into a zeroed 64 KiB slot of HBM (whole words stored, the words shared by two bit ranges OR-ed with global atomics);
//   host    plain arrays, one "thread".
// uq_bgzf_compress works through the blocks in chunks: compress every block of the chunk into its slot, scan the sizes, copy the members
// into place at their 64-bit offsets; the workspace is bounded by the chunk, not by the stream.
//
// LDS: UqDeflateLds is about 151 KiB (the block, one match-length byte per position, the head table / parse window / Huffman scratch, the
// code tables): one workgroup of UQ_DEF_THREADS threads per CU.
#include "common.h"
#include "deflate_core.h"

#define UQ_DEF_THREADS 512
#define UQ_DEF_CHUNK 2048u                   // blocks per pass: 2048 x (64 KiB slot + 127.5 KiB distances) = 383 MiB of workspace
#define UQ_DEF_SLOT 65536u

namespace {

struct X2nArg { uint32_t v[32]; };

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

__global__ __launch_bounds__(UQ_DEF_THREADS) void bgzf_deflate_kernel(const uint8_t* __restrict__ in, uint64_t nbytes, uint64_t first_block,
                                                                      uint8_t* __restrict__ slots, uint16_t* __restrict__ dist,
                                                                      uint32_t* __restrict__ sizes, uint32_t* __restrict__ status, X2nArg x2n) {
    __shared__ __attribute__((aligned(16))) UqDeflateLds s;
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
    const int st = uq_deflate_block(env, &s, n, UQ_DEF_SLOT, tid, UQ_DEF_THREADS, &mb);
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
    UQ_REQUIRE(!(flags & ~(uint32_t)UQ_BGZF_EOF), "uq_bgzf_compress: unknown flags 0x%x", flags);
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
        X2nArg x2n;
        uq_crc_x2n_init(x2n.v);
        uint32_t* h_status = new uint32_t[chunk];
        for (uint64_t b0 = 0; b0 < nblocks; b0 += chunk) {
            const uint32_t nb = (uint32_t)(nblocks - b0 < chunk ? nblocks - b0 : chunk);
            hipError_t e = hipMemsetAsync(slots, 0, (size_t)nb * UQ_DEF_SLOT, c->stream);
            if (e == hipSuccess) {
                bgzf_deflate_kernel<<<nb, UQ_DEF_THREADS, 0, c->stream>>>(d_in, nbytes, b0, slots, dist, sizes, status, x2n);
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

extern "C" int uq_bgzf_compress_block_host(const uint8_t* h_in, uint64_t nbytes, uint8_t* h_out, uint64_t capacity, uint64_t* h_out_bytes,
                                           uint32_t* h_status) {
    UQ_REQUIRE(h_out_bytes && h_status && (h_in || !nbytes) && (h_out || !capacity), "uq_bgzf_compress_block_host: null argument");
    *h_out_bytes = 0;
    if (nbytes > UQ_DEF_MAX_IN) { *h_status = UQ_DEF_TOO_LARGE; return 0; }
    UqDeflateLds* s = new UqDeflateLds();
    uint16_t* dist = new uint16_t[UQ_DEF_MAX_IN];
    uint32_t x2n[32];
    uq_crc_x2n_init(x2n);
    if (nbytes) memcpy(s->in, h_in, nbytes);
    const uint32_t cap = (uint32_t)(capacity < UQ_DEF_SLOT ? capacity : UQ_DEF_SLOT);
    if (cap) memset(h_out, 0, cap);
    HostEnv env{h_out, cap, dist, x2n};
    uint32_t mb = 0;
    const int st = uq_deflate_block(env, s, (uint32_t)nbytes, cap, 0, 1, &mb);
    delete[] dist;
    delete s;
    *h_status = (uint32_t)st;
    *h_out_bytes = mb;
    return 0;
}
