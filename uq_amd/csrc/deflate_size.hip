// deflate_size.hip -- the size a buffer would have as BGZF from this library's own compressor, and no member written: uq_deflate_size (a
// device buffer behind a short host prefix, one workgroup per 65 280-byte block, the block sizes summed on the device) and the host run of
// the same code (uq_deflate_size_host).  What `--test --device-compressor` ranks its candidates by.
//
// The sizer is deflate_core.h's size-only path (uq_deflate_block_size): the compressor's matches, parse, histograms and code lengths, then
// the bit count from the histograms.  Here it gets its two environments:
//   device  the block in LDS, one distance symbol per position in an HBM workspace (65 280 bytes per workgroup);
//   host    plain arrays, one "thread".
// One launch sizes the whole buffer: UQ_SIZE_GRID workgroups at most, each taking every UQ_SIZE_GRID-th block, so the workspace does not
// grow with the buffer; a workgroup adds the sum of its blocks to the caller's 64-bit total with one atomic.  Nothing is read back and the
// stream is not synchronised: calls can be queued back to back and their totals fetched once.
//
// LDS: UqDeflateSizeLds is about 147 KiB (the block, one match-length byte per position, the head table / parse window / Huffman scratch,
// the code lengths): one workgroup of UQ_SIZE_THREADS threads per CU.  Level 2 (the _l entries with UQ_BGZF_LEVEL2: UqDeflateSizeLds2)
// adds 1 KiB and uses the same workspace.
#include "common.h"
#include "deflate_core.h"

#define UQ_SIZE_THREADS 512
#define UQ_SIZE_GRID 2048u                   // workgroups (and distance-symbol slots: 2048 x 65 280 B = 127.5 MiB of workspace)
#define UQ_SIZE_MAX_PREFIX 256u

namespace {

struct PrefixArg { uint32_t w[UQ_SIZE_MAX_PREFIX / 4]; };

struct DevSizeEnv {
    uint8_t* dist;              // the workgroup's distance symbols
    __device__ void sync() { __syncthreads(); }
    __device__ void lds_max(uint32_t* p, uint32_t v) { atomicMax(p, v); }
    __device__ void lds_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
    __device__ void dist_put(uint32_t p, uint32_t sym) { dist[p] = (uint8_t)sym; }
    __device__ uint32_t dist_get(uint32_t p) const { return dist[p]; }
};

template <int kLevel> struct SizeLdsOf { typedef UqDeflateSizeLds type; };
template <> struct SizeLdsOf<2> { typedef UqDeflateSizeLds2 type; };

// blocks are cut on prefix || data: block b holds bytes [b * 65 280, ...) of the concatenation
template <int kLevel>
__global__ __launch_bounds__(UQ_SIZE_THREADS) void deflate_size_kernel(const uint8_t* __restrict__ data, uint64_t nbytes, uint32_t prefix_bytes,
                                                                       uint64_t nblocks, uint8_t* __restrict__ dist,
                                                                       unsigned long long* __restrict__ total, uint32_t* __restrict__ status,
                                                                       PrefixArg prefix) {
    __shared__ __attribute__((aligned(16))) typename SizeLdsOf<kLevel>::type s;
    const uint32_t tid = threadIdx.x;
    const uint64_t all = (uint64_t)prefix_bytes + nbytes;
    DevSizeEnv env{dist + (uint64_t)blockIdx.x * UQ_DEF_MAX_IN};
    unsigned long long sum = 0;
    uint32_t bad = 0;
    for (uint64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const uint64_t off = b * (uint64_t)UQ_DEF_MAX_IN;
        const uint32_t n = (uint32_t)(all - off < UQ_DEF_MAX_IN ? all - off : UQ_DEF_MAX_IN);
        // the prefix (at most 256 bytes) lies inside block 0: in[0, lo) from the kernel argument, in[lo, n) from the buffer
        const uint32_t lo = off < prefix_bytes ? ((uint32_t)(prefix_bytes - off) < n ? (uint32_t)(prefix_bytes - off) : n) : 0;
        if (tid < lo) s.in[tid] = (uint8_t)(prefix.w[tid >> 2] >> (8 * (tid & 3)));
        const uint8_t* src = data + (ptrdiff_t)(off - prefix_bytes);             // src[i] = byte i of the block, for i >= lo
        uint32_t i0 = lo;
        if ((((uintptr_t)src | lo) & 15) == 0) {
            const uint32_t nv = n / 16;
            for (uint32_t v = lo / 16 + tid; v < nv; v += UQ_SIZE_THREADS) ((uint4*)s.in)[v] = ((const uint4*)src)[v];
            i0 = nv * 16;
        }
        for (uint32_t i = i0 + tid; i < n; i += UQ_SIZE_THREADS) s.in[i] = src[i];
        __syncthreads();
        uint32_t mb = 0;
        const int st = uq_deflate_block_size_l<kLevel>(env, &s, n, tid, UQ_SIZE_THREADS, &mb);
        if (st == UQ_DEF_OK) sum += mb; else bad = (uint32_t)st;
        __syncthreads();                                                         // the next block overwrites what was just read
    }
    if (tid == 0) {
        if (sum) atomicAdd(total, sum);
        if (bad) atomicMax(status, bad);
    }
}

struct HostSizeEnv {
    uint8_t* dist;
    void sync() {}
    void lds_max(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
    void lds_add(uint32_t* p, uint32_t v) { *p += v; }
    void dist_put(uint32_t p, uint32_t sym) { dist[p] = (uint8_t)sym; }
    uint32_t dist_get(uint32_t p) const { return dist[p]; }
};

}  // namespace

static int size_device(uq_ctx* c, const uint8_t* h_prefix, uint32_t prefix_bytes, const uint8_t* d_data, uint64_t nbytes, uint64_t* d_total,
                       uint32_t* d_status, uint32_t flags, const char* who) {
    UQ_REQUIRE(c && d_total && d_status, "%s: null argument", who);
    UQ_REQUIRE((h_prefix || !prefix_bytes) && (d_data || !nbytes), "%s: null buffer", who);
    UQ_REQUIRE(prefix_bytes <= UQ_SIZE_MAX_PREFIX, "%s: a prefix of %u bytes (at most %u)", who, prefix_bytes, UQ_SIZE_MAX_PREFIX);
    UQ_REQUIRE(nbytes <= UINT64_MAX - UQ_SIZE_MAX_PREFIX - UQ_DEF_MAX_IN, "%s: nbytes out of range", who);
    UQ_REQUIRE(!(flags & ~(uint32_t)UQ_BGZF_LEVEL2), "%s: unknown flags 0x%x", who, flags);
    const uint64_t nblocks = ((uint64_t)prefix_bytes + nbytes + UQ_DEF_MAX_IN - 1) / UQ_DEF_MAX_IN;
    if (!nblocks) return 0;
    const uint32_t grid = (uint32_t)(nblocks < UQ_SIZE_GRID ? nblocks : UQ_SIZE_GRID);
    void* ws;
    UQ_TRY(uq_scratch(c, (size_t)grid * UQ_DEF_MAX_IN, &ws));
    PrefixArg prefix;
    memset(&prefix, 0, sizeof(prefix));
    if (prefix_bytes) memcpy(prefix.w, h_prefix, prefix_bytes);
    if (flags & UQ_BGZF_LEVEL2)
        deflate_size_kernel<2><<<grid, UQ_SIZE_THREADS, 0, c->stream>>>(d_data, nbytes, prefix_bytes, nblocks, (uint8_t*)ws,
                                                                        (unsigned long long*)d_total, d_status, prefix);
    else
        deflate_size_kernel<1><<<grid, UQ_SIZE_THREADS, 0, c->stream>>>(d_data, nbytes, prefix_bytes, nblocks, (uint8_t*)ws,
                                                                        (unsigned long long*)d_total, d_status, prefix);
    UQ_LAUNCH_CHECK();
    return 0;
}

template <int kLevel>
static uint64_t size_host(const uint8_t* h_prefix, uint32_t prefix_bytes, const uint8_t* h_data, uint64_t all) {
    typedef typename SizeLdsOf<kLevel>::type Lds;
    Lds* s = new Lds();
    uint8_t* dist = new uint8_t[UQ_DEF_MAX_IN];
    HostSizeEnv env{dist};
    uint64_t total = 0;
    for (uint64_t off = 0; off < all; off += UQ_DEF_MAX_IN) {
        const uint32_t n = (uint32_t)(all - off < UQ_DEF_MAX_IN ? all - off : UQ_DEF_MAX_IN);
        const uint32_t lo = off < prefix_bytes ? ((uint32_t)(prefix_bytes - off) < n ? (uint32_t)(prefix_bytes - off) : n) : 0;
        if (lo) memcpy(s->in, h_prefix + off, lo);
        if (n > lo) memcpy(s->in + lo, h_data + (off + lo - prefix_bytes), n - lo);
        uint32_t mb = 0;
        uq_deflate_block_size_l<kLevel>(env, s, n, 0, 1, &mb);
        total += mb;
    }
    delete[] dist;
    delete s;
    return total;
}

static int size_host_checked(const uint8_t* h_prefix, uint32_t prefix_bytes, const uint8_t* h_data, uint64_t nbytes, uint64_t* h_total,
                             uint32_t flags, const char* who) {
    UQ_REQUIRE(h_total && (h_prefix || !prefix_bytes) && (h_data || !nbytes), "%s: null argument", who);
    UQ_REQUIRE(prefix_bytes <= UQ_SIZE_MAX_PREFIX, "%s: a prefix of %u bytes (at most %u)", who, prefix_bytes, UQ_SIZE_MAX_PREFIX);
    UQ_REQUIRE(nbytes <= UINT64_MAX - UQ_SIZE_MAX_PREFIX - UQ_DEF_MAX_IN, "%s: nbytes out of range", who);
    UQ_REQUIRE(!(flags & ~(uint32_t)UQ_BGZF_LEVEL2), "%s: unknown flags 0x%x", who, flags);
    *h_total = 0;
    const uint64_t all = (uint64_t)prefix_bytes + nbytes;
    if (!all) return 0;
    *h_total = flags & UQ_BGZF_LEVEL2 ? size_host<2>(h_prefix, prefix_bytes, h_data, all) : size_host<1>(h_prefix, prefix_bytes, h_data, all);
    return 0;
}

extern "C" int uq_deflate_size(uq_ctx* c, const uint8_t* h_prefix, uint32_t prefix_bytes, const uint8_t* d_data, uint64_t nbytes,
                               uint64_t* d_total, uint32_t* d_status) {
    return size_device(c, h_prefix, prefix_bytes, d_data, nbytes, d_total, d_status, 0, "uq_deflate_size");
}

extern "C" int uq_deflate_size_l(uq_ctx* c, const uint8_t* h_prefix, uint32_t prefix_bytes, const uint8_t* d_data, uint64_t nbytes,
                                 uint64_t* d_total, uint32_t* d_status, uint32_t flags) {
    return size_device(c, h_prefix, prefix_bytes, d_data, nbytes, d_total, d_status, flags, "uq_deflate_size_l");
}

extern "C" int uq_deflate_size_host(const uint8_t* h_prefix, uint32_t prefix_bytes, const uint8_t* h_data, uint64_t nbytes, uint64_t* h_total) {
    return size_host_checked(h_prefix, prefix_bytes, h_data, nbytes, h_total, 0, "uq_deflate_size_host");
}

extern "C" int uq_deflate_size_host_l(const uint8_t* h_prefix, uint32_t prefix_bytes, const uint8_t* h_data, uint64_t nbytes, uint64_t* h_total,
                                      uint32_t flags) {
    return size_host_checked(h_prefix, prefix_bytes, h_data, nbytes, h_total, flags, "uq_deflate_size_host_l");
}
