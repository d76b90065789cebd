// inflate.hip -- gzip input: the member scan on the host (uq_gzip_scan) and the inflate of BGZF members on the device
// (uq_inflate_members, one wave per member), plus the host run of the same decoder on one member (uq_inflate_member_host).
//
// The decoder itself is inflate_core.h.  Here it gets its two environments (the sources and the CRC plumbing are inflate_env.h's, shared with
// inflate_stream.hip):
//   device  Src = DevSrc<uint32_t>; Out = the member's whole output (<= 64 KiB) in LDS, so that back-references read
//                 LDS only and never HBM the kernel has just written; matches are copied by the lanes (src = dst - dist + i % dist), the
//                 output is then CRC-checked by the lanes (per-segment CRCs combined with shift operators) and flushed to HBM with 16-byte
//                 stores.
//   host    plain byte pointers, one "lane".
//
// LDS against occupancy: 64 KiB of output + 5 KiB of code tables + the 1 KiB CRC table = 71 616 bytes a workgroup of one wave, so two members
// are in flight per CU (160 KiB).  A 32 KiB window ring would allow four, at the price of flushing and CRC-ing the ring as it wraps; the
// whole-member buffer keeps the flush one coalesced pass and the CRC one parallel pass (DESIGN.md section 13 has the measurement).
#include "inflate_env.h"

namespace {

struct DevOut {
    uint8_t* o;                 // LDS, the member's output
    const uint8_t* src;         // the member's compressed bytes (stored blocks)
    uint32_t lane;
    __device__ void order() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }
    __device__ void put(uint32_t pos, uint8_t b) {
        if (lane == 0) o[pos] = b;
        order();
    }
    __device__ void copy(uint32_t pos, uint32_t dist, uint32_t len) {
        // every source byte lies below pos: written before this copy, never by it
        if (dist >= 64) {
            for (uint32_t i = lane; i < len; i += 64) o[pos + i] = o[pos - dist + i];
        } else {
            for (uint32_t i = lane; i < len; i += 64) o[pos + i] = o[pos - dist + i % dist];
        }
        order();
    }
    __device__ void stored(uint32_t pos, uint32_t at, uint32_t len) {
        for (uint32_t i = lane; i < len; i += 64) o[pos + i] = src[at + i];
        order();
    }
    __device__ void sync() { __syncthreads(); }
};

__global__ __launch_bounds__(64) void inflate_members_kernel(const uint8_t* __restrict__ comp, uint64_t comp_bytes,
                                                             const uq_gzip_member* __restrict__ members, uint8_t* __restrict__ out,
                                                             uint64_t out_bytes, uint32_t* __restrict__ status, X2n x2n) {
    __shared__ __attribute__((aligned(16))) uint8_t obuf[UQ_INF_MAX_OUT];
    __shared__ UqInflateTables tab;
    __shared__ uint32_t crctab[256];
    const uint32_t lane = threadIdx.x;
    const uint64_t m = blockIdx.x;
    const uq_gzip_member mem = members[m];
    int st = UQ_INF_OK;
    if (mem.isize > UQ_INF_MAX_OUT || mem.comp_bytes > 0xFFFFFFF0ull || mem.data_offset > comp_bytes ||
        mem.comp_bytes > comp_bytes - mem.data_offset || mem.out_offset > out_bytes || mem.isize > out_bytes - mem.out_offset)
        st = UQ_INF_TOO_LARGE;
    if (st == UQ_INF_OK) {
        for (uint32_t e = lane; e < 256; e += 64) crctab[e] = uq_crc_table_entry(e);
        const uint8_t* src = comp + mem.data_offset;
        DevSrc<uint32_t> s{src, (uint32_t)mem.comp_bytes, 0, 0, lane};
        s.load(0);
        DevOut o{obuf, src, lane};
        st = uq_inflate_core(s, (uint32_t)mem.comp_bytes, o, mem.isize, &tab, lane, 64);
        __syncthreads();
    }
    if (st == UQ_INF_OK) {
        // CRC-32: lane l takes bytes [l S, (l + 1) S) (S / 4 odd: the lanes' dword reads fall in different banks), shifted over the rest
        const uint32_t n = mem.isize;
        uint32_t S = (((n + 63) / 64) + 3) & ~3u;
        if (!((S >> 2) & 1)) S += 4;
        const uint32_t lo = min(n, lane * S), hi = min(n, lo + S);
        const uint32_t c = wave_crc0(crctab, x2n, 0, obuf + lo, hi - lo, n - hi);
        if (uq_crc_finish(x2n.v, c, n) != mem.crc32) st = UQ_INF_CRC_MISMATCH;
    }
    if (st == UQ_INF_OK) {
        uint8_t* dst = out + mem.out_offset;
        const uint32_t n = mem.isize;
        uint32_t i0 = 0;
        if (((uintptr_t)dst & 15) == 0) {
            const uint32_t nv = n / 16;
            for (uint32_t v = lane; v < nv; v += 64) ((uint4*)dst)[v] = ((const uint4*)obuf)[v];
            i0 = nv * 16;
        }
        for (uint32_t i = i0 + lane; i < n; i += 64) dst[i] = obuf[i];
    }
    if (lane == 0) status[m] = (uint32_t)st;
}

struct HostOut {
    uint8_t* o;
    const uint8_t* src;
    void put(uint32_t pos, uint8_t b) { o[pos] = b; }
    void copy(uint32_t pos, uint32_t dist, uint32_t len) { for (uint32_t i = 0; i < len; ++i) o[pos + i] = o[pos - dist + i]; }
    void stored(uint32_t pos, uint32_t at, uint32_t len) { if (len) memcpy(o + pos, src + at, len); }
    void sync() {}
};

uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

uint32_t host_crc32(const uint8_t* p, uint64_t n) {
    return uq_crc0_bytes(crc_table(), 0xFFFFFFFFu, p, (uint32_t)n) ^ 0xFFFFFFFFu;
}

}  // namespace

extern "C" int uq_gzip_scan(const uint8_t* h_buf, uint64_t nbytes, uq_gzip_member* h_members, uint64_t capacity, uint64_t* h_nmembers,
                            uint64_t* h_total_out, int* h_kind, uint64_t* h_bad_offset) {
    UQ_REQUIRE(h_nmembers && h_total_out && h_kind && h_bad_offset && (h_buf || !nbytes), "uq_gzip_scan: null argument");
    uint64_t off = 0, n = 0, total = 0;
    int kind = UQ_GZIP_BGZF;
    *h_nmembers = 0; *h_total_out = 0; *h_bad_offset = 0;
#define MALFORMED(...) do { uq_set_error(__VA_ARGS__); *h_kind = UQ_GZIP_MALFORMED; *h_bad_offset = off; *h_nmembers = n;    \
                            *h_total_out = total; return 0; } while (0)
    if (nbytes == 0) MALFORMED("gzip input is empty");
    while (off < nbytes) {
        const uint8_t* b = h_buf + off;
        const uint64_t left = nbytes - off;
        if (left < 10) MALFORMED("gzip member %llu at offset %llu: truncated header", (unsigned long long)n, (unsigned long long)off);
        if (b[0] != 0x1f || b[1] != 0x8b) MALFORMED("gzip member %llu at offset %llu: no gzip magic", (unsigned long long)n, (unsigned long long)off);
        if (b[2] != 8) MALFORMED("gzip member %llu at offset %llu: compression method %d is not deflate", (unsigned long long)n,
                                 (unsigned long long)off, (int)b[2]);
        const uint32_t flg = b[3];
        if (flg & 0xE0) MALFORMED("gzip member %llu at offset %llu: reserved flag bits set", (unsigned long long)n, (unsigned long long)off);
        uint64_t p = 10;
        int64_t bsize = -1;
        if (flg & 4) {                                                  // FEXTRA: subfields SI1 SI2 LEN(2) data
            if (left - p < 2) MALFORMED("gzip member %llu at offset %llu: truncated extra field", (unsigned long long)n, (unsigned long long)off);
            const uint64_t xlen = le16(b + p);
            p += 2;
            if (left - p < xlen) MALFORMED("gzip member %llu at offset %llu: truncated extra field", (unsigned long long)n, (unsigned long long)off);
            uint64_t q = p;
            const uint64_t end = p + xlen;
            while (q < end) {
                if (end - q < 4) MALFORMED("gzip member %llu at offset %llu: malformed extra subfield", (unsigned long long)n, (unsigned long long)off);
                const uint64_t slen = le16(b + q + 2);
                if (end - q - 4 < slen) MALFORMED("gzip member %llu at offset %llu: malformed extra subfield", (unsigned long long)n, (unsigned long long)off);
                if (b[q] == 'B' && b[q + 1] == 'C' && slen == 2) bsize = le16(b + q + 4);
                q += 4 + slen;
            }
            p = end;
        }
        for (uint32_t f = 8; f <= 16; f <<= 1) {                         // FNAME, FCOMMENT: zero-terminated
            if (!(flg & f)) continue;
            const void* z = p < left ? memchr(b + p, 0, left - p) : nullptr;
            if (!z) MALFORMED("gzip member %llu at offset %llu: truncated %s", (unsigned long long)n, (unsigned long long)off,
                              f == 8 ? "file name" : "comment");
            p = (uint64_t)((const uint8_t*)z - b) + 1;
        }
        if (flg & 2) {                                                  // FHCRC: the low 16 bits of the header's CRC-32
            if (left - p < 2) MALFORMED("gzip member %llu at offset %llu: truncated header CRC", (unsigned long long)n, (unsigned long long)off);
            if ((host_crc32(b, p) & 0xFFFF) != le16(b + p))
                MALFORMED("gzip member %llu at offset %llu: header CRC mismatch", (unsigned long long)n, (unsigned long long)off);
            p += 2;
        }
        uq_gzip_member mem;
        mem.data_offset = off + p;
        mem.out_offset = total;
        if (bsize >= 0) {
            const uint64_t msize = (uint64_t)bsize + 1;
            if (msize > left) MALFORMED("gzip member %llu at offset %llu: BSIZE %llu past the end of the input", (unsigned long long)n,
                                        (unsigned long long)off, (unsigned long long)bsize);
            if (msize < p + 8) MALFORMED("gzip member %llu at offset %llu: BSIZE %llu smaller than its header and trailer", (unsigned long long)n,
                                         (unsigned long long)off, (unsigned long long)bsize);
            mem.comp_bytes = msize - 8 - p;
            mem.crc32 = le32(b + msize - 8);
            mem.isize = le32(b + msize - 4);
            if (mem.isize > UQ_INF_MAX_OUT) MALFORMED("gzip member %llu at offset %llu: ISIZE %u > 65536 in a BGZF member", (unsigned long long)n,
                                                      (unsigned long long)off, mem.isize);
            total += mem.isize;
            off += msize;
        } else {
            // no BSIZE: where this member ends is found only by inflating it -- the walk stops here
            if (left - p < 10) MALFORMED("gzip member %llu at offset %llu: truncated member", (unsigned long long)n, (unsigned long long)off);
            mem.comp_bytes = left - p;
            mem.crc32 = 0;
            mem.isize = 0;
            kind = UQ_GZIP_OTHER;
        }
        if (h_members) {
            UQ_REQUIRE(n < capacity, "uq_gzip_scan: more than %llu members (capacity)", (unsigned long long)capacity);
            h_members[n] = mem;
        }
        ++n;
        if (kind == UQ_GZIP_OTHER) break;
    }
#undef MALFORMED
    *h_nmembers = n;
    *h_total_out = total;
    *h_kind = kind;
    return 0;
}

extern "C" int uq_inflate_members(uq_ctx* c, const uint8_t* d_comp, uint64_t comp_bytes, const uq_gzip_member* d_members, uint64_t nmembers,
                                  uint8_t* d_out, uint64_t out_bytes, uint32_t* d_status) {
    UQ_REQUIRE(c, "null context");
    UQ_REQUIRE(nmembers < (1ull << 31), "uq_inflate_members: %llu members (at most 2^31 - 1)", (unsigned long long)nmembers);
    if (nmembers == 0) return 0;
    UQ_REQUIRE(d_comp && d_members && d_status && (d_out || !out_bytes), "uq_inflate_members: null argument");
    X2n x2n;
    uq_crc_x2n_init(x2n.v);
    inflate_members_kernel<<<(uint32_t)nmembers, 64, 0, c->stream>>>(d_comp, comp_bytes, d_members, d_out, out_bytes, d_status, x2n);
    UQ_LAUNCH_CHECK();
    return 0;
}

extern "C" int uq_inflate_member_host(const uint8_t* h_comp, uint64_t comp_bytes, uint8_t* h_out, uint64_t isize, uint32_t crc32,
                                      uint32_t* h_status) {
    UQ_REQUIRE(h_status && (h_comp || !comp_bytes) && (h_out || !isize), "uq_inflate_member_host: null argument");
    if (isize > UQ_INF_MAX_OUT || comp_bytes > 0xFFFFFFF0ull) { *h_status = UQ_INF_TOO_LARGE; return 0; }
    UqInflateTables* t = new UqInflateTables();
    HostSrc<uint32_t> s{h_comp, (uint32_t)comp_bytes};
    HostOut o{h_out, h_comp};
    int st = uq_inflate_core(s, (uint32_t)comp_bytes, o, (uint32_t)isize, t, 0, 1);
    delete t;
    if (st == UQ_INF_OK) {
        // the kernel's CRC arithmetic: crc0 of two segments, the first carried over the second, then the gzip start and inversion
        uint32_t x2n[32];
        uq_crc_x2n_init(x2n);
        const uint32_t half = (uint32_t)isize / 2;
        const uint32_t a = uq_crc0_bytes(crc_table(), 0, h_out, half), b = uq_crc0_bytes(crc_table(), 0, h_out + half, (uint32_t)isize - half);
        const uint32_t c0 = uq_crc_multmodp(uq_crc_shift_op(x2n, isize - half), a) ^ b;
        if (uq_crc_finish(x2n, c0, isize) != crc32) st = UQ_INF_CRC_MISMATCH;
    }
    *h_status = (uint32_t)st;
    return 0;
}
