// inflate_stream.hip -- gzip that is not BGZF, inflated in parallel chunks (the decoder is inflate_stream.h).
//
//   find      gzs_find_kernel: one wave per chunk scans the chunk's bit offsets in order, 64 at a time (one per lane): the cheap tests of
//             uq_gzs_probe_cheap for every offset, the full dynamic-header decode only on the lanes that pass them; the smallest offset that
//             passes wins.  Chunk 0 starts at the first member's header.
//   decode    gzs_decode_kernel: one wave per chunk, symbol decode wave-uniform as in inflate_members_kernel; the 32 KiB window ring of u16
//             symbols in LDS, flushed to the chunk's slot in HBM with 16-byte stores.  Rounds: after each, the host reads the chunk records
//             back and runs the chain check (run_chain): a chunk's speculative result is used only when its predecessor is verified and
//             ended exactly at its start; otherwise it is decoded again from that end, which is a true unit boundary.  Chunks whose slot
//             overflowed are decoded again with a larger slot (grow_cap).  Normally there is one round; finder false positives add one.
//   finish    gzs_compact_kernel places every chunk's symbols at its prefix-summed output offset (markers as placeholders);
//             gzs_windows_kernel carries the 32 KiB windows from chunk to chunk in LDS (one workgroup, in order), resolving the chunks'
//             last 32 KiB; then gzs_resolve_kernel replaces the rest of the markers in parallel; gzs_crc_pieces_kernel
//             and gzs_crc_members_kernel check every member's CRC-32, the host its ISIZE.
// The host entry uq_gzip_stream_host runs the same finder, chunk decoder, chain check and resolution serially.
#include <chrono>
#include <vector>
#include <algorithm>
#include <stdlib.h>
#include "inflate_env.h"
#include "inflate_stream.h"

struct uq_gzip_stream;

namespace {

const char* gzs_status_text(uint32_t st) {
    switch (st) {
        case UQ_INF_TRUNCATED: return "the deflate stream ends early (truncated file)";
        case UQ_INF_BAD_BLOCK_TYPE: return "invalid block type";
        case UQ_INF_BAD_STORED_LEN: return "stored block length check failed";
        case UQ_INF_BAD_CODE_LENGTHS: return "invalid code lengths set";
        case UQ_INF_BAD_REPEAT: return "invalid code length repeat";
        case UQ_INF_BAD_SYMBOL: return "invalid Huffman code";
        case UQ_INF_BAD_DISTANCE: return "invalid distance too far back";
        case UQ_INF_ISIZE_MISMATCH: return "member length != the trailer's ISIZE";
        case UQ_INF_CRC_MISMATCH: return "CRC-32 mismatch";
        case UQ_INF_BAD_COUNTS: return "too many length or distance symbols";
        case UQ_GZS_BAD_HEADER: return "bytes that are not a gzip member header";
        case UQ_GZS_TOO_FAR_BACK: return "invalid distance too far back";
        default: return "corrupt deflate data";
    }
}

// ------------------------------------------------------------------ device
struct DevEnv {
    __device__ void order() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }
    __device__ bool any(bool b) { return __ballot(b) != 0; }
    __device__ void sync() { __syncthreads(); }
    __device__ void store16(uint8_t* d, const uint32_t* w) { *(uint4*)d = make_uint4(w[0], w[1], w[2], w[3]); }
};

__global__ __launch_bounds__(64) void gzs_find_kernel(const uint8_t* __restrict__ comp, uint64_t n, uint64_t chunk_bytes,
                                                      uint64_t* __restrict__ found) {
    __shared__ UqGzsProbe probe[64];
    const uint32_t lane = threadIdx.x;
    const uint64_t k = (uint64_t)blockIdx.x + 1;
    const uint64_t lo = 8 * k * chunk_bytes, hi = min(8 * (k + 1) * chunk_bytes, 8 * n);
    HostSrc<uint64_t> s{comp, n};
    uint64_t res = UQ_GZS_NONE;
    for (uint64_t base = lo; base < hi; base += 64) {
        const uint64_t b = base + lane;
        uint64_t mine = UQ_GZS_NONE;
        if (b < hi) {
            const uint32_t m = uq_gzs_probe_cheap(s, n, b);
            if (m & 1) mine = b << 2 | UQ_GZS_MEMBER;
            else if (m & 2) mine = b << 2 | UQ_GZS_UNCOMPRESSED;
            else if ((m & 4) && uq_gzs_probe_dynamic(s, n, b, &probe[lane])) mine = b << 2 | UQ_GZS_DYNAMIC;
        }
        const uint64_t bal = __ballot(mine != UQ_GZS_NONE);
        if (bal) {
            const int first = __builtin_ctzll(bal);
            const uint32_t rlo = __shfl((uint32_t)mine, first, 64), rhi = __shfl((uint32_t)(mine >> 32), first, 64);
            res = (uint64_t)rhi << 32 | rlo;
            break;
        }
    }
    if (lane == 0) found[k] = res;
}

// LDS: the ring 65 536 bytes + code tables 5 KiB + CRC table 1 KiB (member header CRCs) -> two waves per CU
__global__ __launch_bounds__(64) void gzs_decode_kernel(const uint8_t* __restrict__ comp, uint64_t n, UqGzsChunk* chunks,
                                                        const uint32_t* __restrict__ todo) {
    __shared__ __attribute__((aligned(16))) uint16_t ring[UQ_GZS_RING];
    __shared__ UqInflateTables tab;
    __shared__ uint32_t crctab[256];
    const uint32_t lane = threadIdx.x;
    for (uint32_t e = lane; e < 256; e += 64) crctab[e] = uq_crc_table_entry(e);
    __syncthreads();
    DevSrc<uint64_t> s{comp, n, 0, 0, lane};
    s.load(0);
    DevEnv env;
    uq_gzs_chunk(s, n, &chunks[todo[blockIdx.x]], ring, &tab, crctab, lane, 64u, env);
}

struct GzsPlace { uint64_t slot, out, len, split, mstart, chunk; };
#define GZS_BLOCKS_PER_CHUNK 8

__global__ __launch_bounds__(256) void gzs_compact_kernel(const GzsPlace* __restrict__ pl, uint8_t* __restrict__ out) {
    const GzsPlace p = pl[blockIdx.x / GZS_BLOCKS_PER_CHUNK];
    const uint16_t* s16 = (const uint16_t*)p.slot;
    const uint8_t* s8 = (const uint8_t*)p.slot + p.split;
    uint8_t* o = out + p.out;
    const uint64_t step = 256ull * GZS_BLOCKS_PER_CHUNK;
    for (uint64_t i = (blockIdx.x % GZS_BLOCKS_PER_CHUNK) * 256ull + threadIdx.x; i < p.len; i += step) {
        uint32_t v;
        if (i < p.split) { v = s16[i]; if (v >= 256) v = 0; }
        else v = s8[i];
        o[i] = (uint8_t)v;
    }
}

// markers of the listed chunks below their last 32 KiB, once every window is final: out[O + i] = out[O - 32768 + w]; a marker before the
// member's start flags the chunk
__global__ __launch_bounds__(256) void gzs_resolve_kernel(const GzsPlace* __restrict__ pl, uint8_t* out, uint32_t* __restrict__ bad) {
    const uint32_t c = blockIdx.x / GZS_BLOCKS_PER_CHUNK;
    const GzsPlace p = pl[c];
    const uint16_t* s16 = (const uint16_t*)p.slot;
    const uint64_t step = 256ull * GZS_BLOCKS_PER_CHUNK;
    bool b = false;
    const uint64_t lim = min(p.split, p.len > UQ_GZS_RING ? p.len - UQ_GZS_RING : 0ull);    // the last 32 KiB: gzs_windows_kernel
    for (uint64_t i = (blockIdx.x % GZS_BLOCKS_PER_CHUNK) * 256ull + threadIdx.x; i < lim; i += step) {
        const uint32_t v = s16[i];
        if (v < 256) continue;
        const uint64_t w = v - 256;
        if (p.out + w < p.mstart + UQ_GZS_RING) { b = true; continue; }
        out[p.out + i] = out[p.out - UQ_GZS_RING + w];
    }
    if (b) atomicOr(&bad[c], 1u);
}

// The windows, in one pass over the chunks in order (one workgroup): the window of chunk k (the 32 KiB of output before it) is kept in LDS;
// chunk k's last 32 KiB are resolved against it (and written out where they held markers) and become, with what is left of the old window
// when the chunk is shorter, the window of chunk k + 1.  After it every window in `out` is final, so the rest of the markers resolve in
// parallel (gzs_resolve_kernel, positions below len - 32 KiB).
__global__ __launch_bounds__(1024) void gzs_windows_kernel(const GzsPlace* __restrict__ pl, uint64_t nc, uint8_t* out, uint32_t* __restrict__ bad) {
    __shared__ uint8_t win[2][UQ_GZS_RING];
    uint32_t cur = 0;
    for (uint32_t j = threadIdx.x; j < UQ_GZS_RING; j += 1024) win[0][j] = 0;
    __syncthreads();
    for (uint64_t k = 0; k < nc; ++k) {
        const GzsPlace p = pl[k];
        const uint16_t* s16 = (const uint16_t*)p.slot;
        const uint8_t* s8 = (const uint8_t*)p.slot + p.split;
        bool b = false;
        for (uint32_t j = threadIdx.x; j < UQ_GZS_RING; j += 1024) {
            const int64_t i = (int64_t)p.len - (int64_t)UQ_GZS_RING + j;            // chunk-relative position of new window byte j
            uint8_t v;
            if (i < 0) v = win[cur][p.len + j];
            else if ((uint64_t)i >= p.split) v = s8[i];
            else {
                const uint32_t x = s16[i];
                if (x < 256) v = (uint8_t)x;
                else {
                    const uint64_t w = x - 256;
                    if (p.out + w < p.mstart + UQ_GZS_RING) b = true;
                    v = win[cur][w];
                    out[p.out + i] = v;
                }
            }
            win[cur ^ 1][j] = v;
        }
        if (b) atomicOr(&bad[k], 1u);
        __syncthreads();
        cur ^= 1;
    }
}

struct GzsPiece { uint64_t off, len; };
struct GzsMemberCheck { uint64_t p0, p1, end, len; uint32_t crc32, reserved; };

// crc0 of each piece (<= 64 KiB of the output): lane segments combined with the shift operators
__global__ __launch_bounds__(64) void gzs_crc_pieces_kernel(const uint8_t* __restrict__ out, const GzsPiece* __restrict__ pc,
                                                            uint32_t* __restrict__ crc, X2n x2n) {
    __shared__ uint32_t tab[256];
    const uint32_t lane = threadIdx.x;
    for (uint32_t e = lane; e < 256; e += 64) tab[e] = uq_crc_table_entry(e);
    __syncthreads();
    const GzsPiece p = pc[blockIdx.x];
    const uint64_t S = (p.len + 63) / 64;
    const uint64_t lo = min(p.len, lane * S), hi = min(p.len, lo + S);
    const uint8_t* b = out + p.off;
    uint32_t c = 0;
    uint64_t i = lo;
    for (; i < hi && ((uintptr_t)(b + i) & 3); ++i) c = tab[(c ^ b[i]) & 0xFF] ^ (c >> 8);
    c = wave_crc0(tab, x2n, c, b + i, (uint32_t)(hi - i), p.len - hi);
    if (lane == 0) crc[blockIdx.x] = c;
}

// one wave per member: its pieces' crc0 carried over the bytes after them, XOR-ed, compared with the trailer
__global__ __launch_bounds__(64) void gzs_crc_members_kernel(const GzsPiece* __restrict__ pc, const uint32_t* __restrict__ pcrc,
                                                             const GzsMemberCheck* __restrict__ mc, uint32_t* __restrict__ bad, X2n x2n) {
    const uint32_t lane = threadIdx.x;
    const GzsMemberCheck m = mc[blockIdx.x];
    uint32_t c = 0;
    for (uint64_t j = m.p0 + lane; j < m.p1; j += 64) {
        const GzsPiece p = pc[j];
        c ^= uq_crc_multmodp(uq_crc_shift_op(x2n.v, m.end - (p.off + p.len)), pcrc[j]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c ^= __shfl_xor(c, d, 64);
    if (lane == 0) bad[blockIdx.x] = uq_crc_finish(x2n.v, c, m.len) != m.crc32;
}

// ------------------------------------------------------------------ host
struct HostEnv {
    void order() {}
    bool any(bool b) { return b; }
    void sync() {}
    void store16(uint8_t* d, const uint32_t* w) { memcpy(d, w, 16); }
};

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

struct uq_gzip_stream {
    uq_ctx* ctx = nullptr;                    // null: the host entry
    const uint8_t* comp = nullptr;
    uint64_t n = 0;
    std::vector<UqGzsChunk> ch;
    std::vector<std::pair<void*, uint64_t>> bufs;   // slot memory (device or host) and its size
    std::vector<UqGzsMember> mem;             // every member's record, in order
    std::vector<uint64_t> mem_end;            // global output offset of each member's end
    std::vector<uint64_t> off;                // output offset of each chunk
    uint64_t total = 0;
    uq_gzip_stream_info info{};
    void release(void* b) {
        if (ctx) (void)hipFree(b);
        else free(b);
    }
    // the slot buffers of earlier rounds that no chunk of the verified chain uses any more
    void release_unused() {
        std::vector<std::pair<void*, uint64_t>> keep;
        for (auto& b : bufs) {
            const uint64_t lo = (uint64_t)(uintptr_t)b.first, hi = lo + b.second;
            bool used = false;
            for (const UqGzsChunk& c : ch) if (c.slot >= lo && c.slot < hi) { used = true; break; }
            if (used) keep.push_back(b);
            else release(b.first);
        }
        bufs.swap(keep);
    }
    ~uq_gzip_stream() {
        for (auto& b : bufs) release(b.first);
    }
};

namespace {

uint64_t pos_of(uint64_t u) { return u >> 2; }

// Slot capacity of a chunk spanning `span` compressed bytes.  A chunk that does not start at a member header keeps its symbols as u16 while
// markers live, and on FASTQ they live to the chunk's end: 16 x span is room for a compression ratio of 8 in u16
// (real FASTQ: 3 - 5), plus the first window.
uint64_t first_cap(uint64_t span) { return ((16 * span + (160u << 10)) + 31) & ~31ull; }

// The slot for a chunk that overflowed: at least twice the old one, and enough for the whole span at the ratio the failed decode saw
// (cap bytes for the compressed bytes it consumed), with a quarter to spare -- so a chunk is rarely decoded more than twice.
uint64_t grow_cap(const UqGzsChunk& c, uint64_t n) {
    const uint64_t b0 = pos_of(c.start) >> 3;
    const uint64_t b1 = c.stop == UQ_GZS_NONE ? n : (c.stop + 7) >> 3;
    const uint64_t span = b1 > b0 ? b1 - b0 : 1;
    const uint64_t used = c.err_byte > b0 ? c.err_byte - b0 : 1;
    const double want = (double)c.cap * ((double)span / (double)used) * 1.25 + (64u << 10);
    uint64_t cap = 2 * c.cap;
    if (want > (double)cap) cap = want < 4.0e12 ? (uint64_t)want : (1ull << 42);
    return (cap + 31) & ~31ull;
}

int file_error(uint32_t* h_status, uint64_t* h_bad, uint32_t st, uint64_t at) {
    *h_status = st;
    *h_bad = at;
    uq_set_error("gzip stream: %s at byte %llu", gzs_status_text(st), (unsigned long long)at);
    return 0;
}

// Decodes the chunks listed in `todo`, their slots allocated here (device: one allocation per round)
int decode_round(uq_gzip_stream* s, const std::vector<uint32_t>& todo) {
    uint64_t bytes = 0;
    for (uint32_t k : todo) bytes += s->ch[k].cap;
    void* buf = nullptr;
    if (s->ctx) {
        if (hipMalloc(&buf, bytes ? bytes : 16) != hipSuccess) {
            (void)hipGetLastError();
            size_t fr = 0, tot = 0;
            (void)hipMemGetInfo(&fr, &tot);
            UQ_REQUIRE(false, "gzip stream: %llu bytes of chunk slots do not fit in device memory (%llu free); --host-inflate inflates on the host",
                       (unsigned long long)bytes, (unsigned long long)fr);
        }
    }
    else {
        buf = aligned_alloc(64, ((bytes ? bytes : 16) + 63) & ~63ull);
        UQ_REQUIRE(buf, "gzip stream: out of host memory (%llu bytes of slots)", (unsigned long long)bytes);
    }
    s->bufs.push_back({buf, bytes ? bytes : 16});
    uint64_t o = 0;
    for (uint32_t k : todo) { s->ch[k].slot = (uint64_t)(uintptr_t)buf + o; o += s->ch[k].cap; }
    if (s->ctx) {
        hipStream_t st = s->ctx->stream;
        UqGzsChunk* d_ch = nullptr;
        uint32_t* d_todo = nullptr;
        UQ_CHECK_HIP(hipMallocAsync((void**)&d_ch, s->ch.size() * sizeof(UqGzsChunk), st));
        UQ_CHECK_HIP(hipMallocAsync((void**)&d_todo, todo.size() * sizeof(uint32_t), st));
        UQ_CHECK_HIP(hipMemcpyAsync(d_ch, s->ch.data(), s->ch.size() * sizeof(UqGzsChunk), hipMemcpyHostToDevice, st));
        UQ_CHECK_HIP(hipMemcpyAsync(d_todo, todo.data(), todo.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        gzs_decode_kernel<<<(uint32_t)todo.size(), 64, 0, st>>>(s->comp, s->n, d_ch, d_todo);
        UQ_LAUNCH_CHECK();
        UQ_CHECK_HIP(hipMemcpyAsync(s->ch.data(), d_ch, s->ch.size() * sizeof(UqGzsChunk), hipMemcpyDeviceToHost, st));
        UQ_CHECK_HIP(hipFreeAsync(d_ch, st));
        UQ_CHECK_HIP(hipFreeAsync(d_todo, st));
        UQ_CHECK_HIP(hipStreamSynchronize(st));
    } else {
        HostSrc<uint64_t> src{s->comp, s->n};
        HostEnv env;
        UqInflateTables* t = new UqInflateTables();
        uint16_t* ring = new uint16_t[UQ_GZS_RING];
        for (uint32_t k : todo) uq_gzs_chunk(src, s->n, &s->ch[k], ring, t, crc_table(), 0u, 1u, env);
        delete[] ring;
        delete t;
    }
    s->info.rounds++;
    if (s->info.rounds > 1) s->info.redecoded += todo.size();
    return 0;
}

// The chain check.  Chunk 0 starts at the first member's header, so it is verified; chunk k + 1's result is used only when chunk k is verified
// and ended exactly at chunk k + 1's start.  Otherwise chunk k + 1 is decoded again from chunk k's end (a true unit boundary, by induction);
// chunks whose start lies before that end are dropped.  A status from an unverified chunk means only "bad start"; from a verified one it is
// a file error.
int run_chain(uq_gzip_stream* s, uint32_t* h_status, uint64_t* h_bad) {
    size_t frontier = 0;                      // chunks [0, frontier) are verified
    for (uint32_t guard = 0;; ++guard) {
        UQ_REQUIRE(guard < 1000000, "gzip stream: the chain check does not converge");
        std::vector<uint32_t> todo;
        bool finished = false;
        size_t i = frontier;
        while (i < s->ch.size()) {
            UqGzsChunk& c = s->ch[i];
            if (c.status == UQ_GZS_OVERFLOW) {
                c.cap = grow_cap(c, s->n);
                UQ_REQUIRE(c.cap < (1ull << 42), "gzip stream: chunk %llu needs more than 4 TiB", (unsigned long long)i);
                todo.push_back((uint32_t)i);
                s->info.overflows++;
                break;
            }
            if (c.status) return file_error(h_status, h_bad, c.status, c.err_byte);
            frontier = i + 1;
            if ((c.end & 3) == UQ_GZS_END) {
                s->ch.resize(i + 1);
                finished = true;
                break;
            }
            size_t j = i + 1;
            while (j < s->ch.size() && (pos_of(s->ch[j].start) < pos_of(c.end) || (pos_of(s->ch[j].start) == pos_of(c.end) && s->ch[j].start != c.end)))
                ++j;
            s->ch.erase(s->ch.begin() + (long)(i + 1), s->ch.begin() + (long)j);
            if (i + 1 < s->ch.size() && s->ch[i + 1].start == c.end) { i = i + 1; continue; }
            // decode again from this chunk's end, up to the next start
            UqGzsChunk nc{};
            nc.start = c.end;
            nc.stop = i + 1 < s->ch.size() ? pos_of(s->ch[i + 1].start) : UQ_GZS_NONE;
            nc.cap = first_cap(((nc.stop == UQ_GZS_NONE ? 8 * s->n : nc.stop) - pos_of(nc.start)) / 8);
            s->ch.insert(s->ch.begin() + (long)(i + 1), nc);
            todo.push_back((uint32_t)(i + 1));
            break;
        }
        if (finished) break;
        UQ_REQUIRE(!todo.empty(), "gzip stream: the last chunk did not reach the end of the data");
        // past the frontier, in the same round, so that they do not cost a round each later: overflowed chunks with a larger slot, and
        // chunks whose predecessor's speculative decode ended elsewhere than at their start, from that end (right if the predecessor is)
        for (size_t k = todo.back() + 1; k < s->ch.size(); ++k) {
            UqGzsChunk& c = s->ch[k];
            const UqGzsChunk& p = s->ch[k - 1];
            const bool pred_fresh = std::find(todo.begin(), todo.end(), (uint32_t)(k - 1)) != todo.end();
            if (c.status == UQ_GZS_OVERFLOW) {
                c.cap = grow_cap(c, s->n);
                if (c.cap < (1ull << 42)) todo.push_back((uint32_t)k);
            } else if (!pred_fresh && p.status == UQ_INF_OK && (p.end & 3) != UQ_GZS_END && p.end != c.start && pos_of(p.end) > pos_of(c.start) &&
                       (k + 1 == s->ch.size() || pos_of(p.end) < pos_of(s->ch[k + 1].start))) {
                c.start = p.end;
                c.cap = first_cap(((c.stop == UQ_GZS_NONE ? 8 * s->n : c.stop) - pos_of(c.start)) / 8);
                todo.push_back((uint32_t)k);
            }
        }
        UQ_TRY(decode_round(s, todo));
    }
    return 0;
}

// Reads back the member records, places the chunks, checks the chain's closure.  Fills s->off, s->total, s->mem, s->mem_end.
int place(uq_gzip_stream* s) {
    const size_t nc = s->ch.size();
    s->off.resize(nc + 1);
    uint64_t o = 0;
    std::vector<uint64_t> moff(nc + 1);
    uint64_t nm = 0;
    for (size_t k = 0; k < nc; ++k) { s->off[k] = o; o += s->ch[k].len; moff[k] = nm; nm += s->ch[k].nmem; }
    s->off[nc] = o; moff[nc] = nm;
    s->total = o;
    s->mem.resize(nm);
    std::vector<UqGzsMember> rev;
    for (size_t k = 0; k < nc; ++k) {                   // a chunk's records lie below its slot's end, the first one highest
        const UqGzsChunk& c = s->ch[k];
        if (!c.nmem) continue;
        rev.resize(c.nmem);
        const void* at = (const void*)(uintptr_t)(c.slot + c.cap - (uint64_t)UQ_GZS_MEMBER_REC * c.nmem);
        if (s->ctx) UQ_CHECK_HIP(hipMemcpy(rev.data(), at, c.nmem * sizeof(UqGzsMember), hipMemcpyDeviceToHost));
        else memcpy(rev.data(), at, c.nmem * sizeof(UqGzsMember));
        for (uint32_t j = 0; j < c.nmem; ++j) s->mem[moff[k] + j] = rev[c.nmem - 1 - j];
    }
    s->mem_end.resize(nm);
    size_t m = 0;
    for (size_t k = 0; k < nc; ++k)
        for (uint32_t j = 0; j < s->ch[k].nmem; ++j, ++m) s->mem_end[m] = s->off[k] + s->mem[m].out_pos;
    s->info.chunks = nc;
    s->info.members = nm;
    s->info.out_bytes = s->total;
    return 0;
}

// the start of the member that holds output offset o (the largest member end <= o, or 0)
uint64_t member_start(const uq_gzip_stream* s, uint64_t o) {
    auto it = std::upper_bound(s->mem_end.begin(), s->mem_end.end(), o);
    return it == s->mem_end.begin() ? 0 : *(it - 1);
}

int begin_common(uq_gzip_stream* s, uint64_t chunk_bytes, const uint64_t* h_starts, uint64_t nstarts, uint32_t* h_status, uint64_t* h_bad) {
    const uint64_t n = s->n;
    std::vector<uint64_t> starts;
    double t0 = now_ms();
    if (h_starts) {
        for (uint64_t i = 0; i < nstarts; ++i) {
            const uint64_t u = h_starts[i];
            if ((u & 3) == UQ_GZS_END || pos_of(u) == 0 || pos_of(u) >= 8 * n) continue;
            if ((u & 3) != UQ_GZS_DYNAMIC && (pos_of(u) & 7)) continue;
            starts.push_back(u);
        }
    } else {
        UQ_REQUIRE(chunk_bytes >= 64, "uq_gzip_stream: chunk_bytes %llu < 64", (unsigned long long)chunk_bytes);
        const uint64_t nch = (n + chunk_bytes - 1) / chunk_bytes;
        std::vector<uint64_t> found(nch, UQ_GZS_NONE);
        if (nch > 1) {
            if (s->ctx) {
                uint64_t* d_found = nullptr;
                UQ_REQUIRE(nch - 1 < (1ull << 31), "uq_gzip_stream: too many chunks");
                UQ_CHECK_HIP(hipMallocAsync((void**)&d_found, nch * sizeof(uint64_t), s->ctx->stream));
                gzs_find_kernel<<<(uint32_t)(nch - 1), 64, 0, s->ctx->stream>>>(s->comp, n, chunk_bytes, d_found);
                UQ_LAUNCH_CHECK();
                UQ_CHECK_HIP(hipMemcpyAsync(found.data() + 1, d_found + 1, (nch - 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s->ctx->stream));
                UQ_CHECK_HIP(hipFreeAsync(d_found, s->ctx->stream));
                UQ_CHECK_HIP(hipStreamSynchronize(s->ctx->stream));
            } else {
                HostSrc<uint64_t> src{s->comp, n};
                UqGzsProbe p;
                for (uint64_t k = 1; k < nch; ++k) found[k] = uq_gzs_find(src, n, 8 * k * chunk_bytes, 8 * (k + 1) * chunk_bytes, &p);
            }
        }
        for (uint64_t k = 1; k < nch; ++k) if (found[k] != UQ_GZS_NONE) starts.push_back(found[k]);   // a chunk with no start merges into its predecessor
    }
    std::sort(starts.begin(), starts.end());
    starts.erase(std::unique(starts.begin(), starts.end(), [](uint64_t a, uint64_t b) { return pos_of(a) == pos_of(b); }), starts.end());
    starts.insert(starts.begin(), (uint64_t)UQ_GZS_MEMBER);
    s->info.starts = starts.size();
    double t1 = now_ms();
    s->info.find_ms = t1 - t0;
    s->ch.resize(starts.size());
    std::vector<uint32_t> todo(starts.size());
    for (size_t k = 0; k < starts.size(); ++k) {
        UqGzsChunk& c = s->ch[k];
        c = UqGzsChunk{};
        c.start = starts[k];
        c.stop = k + 1 < starts.size() ? pos_of(starts[k + 1]) : UQ_GZS_NONE;
        c.cap = first_cap(((c.stop == UQ_GZS_NONE ? 8 * n : c.stop) - pos_of(c.start)) / 8);
        todo[k] = (uint32_t)k;
    }
    UQ_TRY(decode_round(s, todo));
    UQ_TRY(run_chain(s, h_status, h_bad));
    if (*h_status) return 0;
    s->release_unused();
    UQ_TRY(place(s));
    s->info.decode_ms = now_ms() - t1;
    return 0;
}

// ISIZE of every member (host), then the markers, then the CRCs
int check_isize(uq_gzip_stream* s, uint32_t* h_status, uint64_t* h_bad) {
    for (size_t m = 0; m < s->mem.size(); ++m) {
        const uint64_t st = m ? s->mem_end[m - 1] : 0;
        if ((uint32_t)(s->mem_end[m] - st) != s->mem[m].isize) return file_error(h_status, h_bad, UQ_INF_ISIZE_MISMATCH, s->mem[m].trailer);
    }
    return 0;
}

int finish_device(uq_gzip_stream* s, uint8_t* d_out, uint32_t* h_status, uint64_t* h_bad) {
    hipStream_t st = s->ctx->stream;
    const size_t nc = s->ch.size();
    std::vector<GzsPlace> pl(nc);
    std::vector<uint8_t> pending(nc);
    for (size_t k = 0; k < nc; ++k) {
        pl[k] = GzsPlace{s->ch[k].slot, s->off[k], s->ch[k].len, s->ch[k].split, member_start(s, s->off[k]), k};
        pending[k] = s->ch[k].markers && s->ch[k].split;
    }
    std::vector<GzsPlace> rp;                             // the chunks that hold markers
    for (size_t k = 0; k < nc; ++k) if (pending[k]) rp.push_back(pl[k]);
    GzsPlace *d_pl = nullptr, *d_rp = nullptr;
    uint32_t *d_bad = nullptr, *d_rb = nullptr;
    UQ_CHECK_HIP(hipMalloc((void**)&d_pl, nc * sizeof(GzsPlace)));
    UQ_CHECK_HIP(hipMalloc((void**)&d_bad, nc * 4));
    UQ_CHECK_HIP(hipMalloc((void**)&d_rp, std::max<size_t>(1, rp.size()) * sizeof(GzsPlace)));
    UQ_CHECK_HIP(hipMalloc((void**)&d_rb, std::max<size_t>(1, rp.size()) * 4));
    UQ_CHECK_HIP(hipMemcpyAsync(d_pl, pl.data(), nc * sizeof(GzsPlace), hipMemcpyHostToDevice, st));
    UQ_CHECK_HIP(hipMemsetAsync(d_bad, 0, nc * 4, st));
    gzs_compact_kernel<<<(uint32_t)(nc * GZS_BLOCKS_PER_CHUNK), 256, 0, st>>>(d_pl, d_out);
    UQ_LAUNCH_CHECK();
    std::vector<uint32_t> hb(nc), rb(rp.size());
    if (!rp.empty()) {
        UQ_CHECK_HIP(hipMemcpyAsync(d_rp, rp.data(), rp.size() * sizeof(GzsPlace), hipMemcpyHostToDevice, st));
        UQ_CHECK_HIP(hipMemsetAsync(d_rb, 0, rp.size() * 4, st));
        gzs_windows_kernel<<<1, 1024, 0, st>>>(d_pl, nc, d_out, d_bad);
        UQ_LAUNCH_CHECK();
        gzs_resolve_kernel<<<(uint32_t)(rp.size() * GZS_BLOCKS_PER_CHUNK), 256, 0, st>>>(d_rp, d_out, d_rb);
        UQ_LAUNCH_CHECK();
        UQ_CHECK_HIP(hipMemcpyAsync(hb.data(), d_bad, nc * 4, hipMemcpyDeviceToHost, st));
        UQ_CHECK_HIP(hipMemcpyAsync(rb.data(), d_rb, rp.size() * 4, hipMemcpyDeviceToHost, st));
        s->info.resolve_rounds = 1;
    }
    UQ_CHECK_HIP(hipStreamSynchronize(st));
    (void)hipFree(d_pl); (void)hipFree(d_bad); (void)hipFree(d_rp); (void)hipFree(d_rb);
    for (size_t i = 0; i < rp.size(); ++i) if (rb[i]) hb[rp[i].chunk] = 1;
    for (size_t k = 0; k < nc; ++k)
        if (hb[k]) return file_error(h_status, h_bad, UQ_GZS_TOO_FAR_BACK, pos_of(s->ch[k].start) >> 3);
    // CRC-32 of every member: pieces of <= 64 KiB
    std::vector<GzsPiece> pcs;
    std::vector<GzsMemberCheck> mc(s->mem.size());
    for (size_t m = 0; m < s->mem.size(); ++m) {
        const uint64_t a = m ? s->mem_end[m - 1] : 0, b = s->mem_end[m];
        mc[m].p0 = pcs.size();
        for (uint64_t x = a; x < b; x += 65536) pcs.push_back(GzsPiece{x, std::min<uint64_t>(65536, b - x)});
        mc[m].p1 = pcs.size();
        mc[m].end = b; mc[m].len = b - a; mc[m].crc32 = s->mem[m].crc32; mc[m].reserved = 0;
    }
    if (mc.empty()) return 0;
    X2n x2n;
    uq_crc_x2n_init(x2n.v);
    GzsPiece* d_pc = nullptr;
    uint32_t *d_pcrc = nullptr, *d_mbad = nullptr;
    GzsMemberCheck* d_mc = nullptr;
    UQ_CHECK_HIP(hipMalloc((void**)&d_pc, std::max<size_t>(1, pcs.size()) * sizeof(GzsPiece)));
    UQ_CHECK_HIP(hipMalloc((void**)&d_pcrc, std::max<size_t>(1, pcs.size()) * 4));
    UQ_CHECK_HIP(hipMalloc((void**)&d_mc, mc.size() * sizeof(GzsMemberCheck)));
    UQ_CHECK_HIP(hipMalloc((void**)&d_mbad, mc.size() * 4));
    if (!pcs.empty()) {
        UQ_CHECK_HIP(hipMemcpyAsync(d_pc, pcs.data(), pcs.size() * sizeof(GzsPiece), hipMemcpyHostToDevice, st));
        gzs_crc_pieces_kernel<<<(uint32_t)pcs.size(), 64, 0, st>>>(d_out, d_pc, d_pcrc, x2n);
        UQ_LAUNCH_CHECK();
    }
    UQ_CHECK_HIP(hipMemcpyAsync(d_mc, mc.data(), mc.size() * sizeof(GzsMemberCheck), hipMemcpyHostToDevice, st));
    gzs_crc_members_kernel<<<(uint32_t)mc.size(), 64, 0, st>>>(d_pc, d_pcrc, d_mc, d_mbad, x2n);
    UQ_LAUNCH_CHECK();
    std::vector<uint32_t> mbad(mc.size());
    UQ_CHECK_HIP(hipMemcpyAsync(mbad.data(), d_mbad, mc.size() * 4, hipMemcpyDeviceToHost, st));
    UQ_CHECK_HIP(hipStreamSynchronize(st));
    (void)hipFree(d_pc); (void)hipFree(d_pcrc); (void)hipFree(d_mc); (void)hipFree(d_mbad);
    for (size_t m = 0; m < mc.size(); ++m)
        if (mbad[m]) return file_error(h_status, h_bad, UQ_INF_CRC_MISMATCH, s->mem[m].trailer);
    return 0;
}

int finish_host(uq_gzip_stream* s, uint8_t* h_out, uint32_t* h_status, uint64_t* h_bad) {
    const size_t nc = s->ch.size();
    for (size_t k = 0; k < nc; ++k) {                   // in order: every window is final when its chunk is resolved
        const UqGzsChunk& c = s->ch[k];
        const uint8_t* slot = (const uint8_t*)(uintptr_t)c.slot;
        uint8_t* o = h_out + s->off[k];
        const uint64_t ms = member_start(s, s->off[k]);
        for (uint64_t i = 0; i < c.len; ++i) {
            if (i >= c.split) { o[i] = slot[c.split + i]; continue; }
            const uint32_t v = (uint32_t)slot[2 * i] | (uint32_t)slot[2 * i + 1] << 8;
            if (v < 256) { o[i] = (uint8_t)v; continue; }
            const uint64_t w = v - 256;
            if (s->off[k] + w < ms + UQ_GZS_RING) return file_error(h_status, h_bad, UQ_GZS_TOO_FAR_BACK, pos_of(c.start) >> 3);
            o[i] = h_out[s->off[k] - UQ_GZS_RING + w];
        }
        if (c.markers && c.split) s->info.resolve_rounds = 1;
    }
    uint32_t x2n[32];
    uq_crc_x2n_init(x2n);
    for (size_t m = 0; m < s->mem.size(); ++m) {
        const uint64_t a = m ? s->mem_end[m - 1] : 0, b = s->mem_end[m];
        uint32_t c = 0;
        for (uint64_t x = a; x < b; x += 1u << 30) {
            const uint32_t l = (uint32_t)std::min<uint64_t>(1u << 30, b - x);
            c = uq_crc_multmodp(uq_crc_shift_op(x2n, l), c) ^ uq_crc0_bytes(crc_table(), 0, h_out + x, l);
        }
        if (uq_crc_finish(x2n, c, b - a) != s->mem[m].crc32) return file_error(h_status, h_bad, UQ_INF_CRC_MISMATCH, s->mem[m].trailer);
    }
    return 0;
}

}  // namespace

extern "C" int uq_gzip_stream_begin(uq_ctx* c, const uint8_t* d_comp, uint64_t comp_bytes, uint64_t chunk_bytes, const uint64_t* h_starts,
                                    uint64_t nstarts, uq_gzip_stream** h_stream, uint64_t* h_out_bytes, uint32_t* h_status, uint64_t* h_bad_offset) {
    UQ_REQUIRE(c && h_stream && h_out_bytes && h_status && h_bad_offset && (d_comp || !comp_bytes), "uq_gzip_stream_begin: null argument");
    *h_stream = nullptr; *h_out_bytes = 0; *h_status = 0; *h_bad_offset = 0;
    uq_gzip_stream* s = new uq_gzip_stream();
    s->ctx = c; s->comp = d_comp; s->n = comp_bytes;
    int rc = begin_common(s, chunk_bytes, h_starts, nstarts, h_status, h_bad_offset);
    if (rc || *h_status) { delete s; return rc; }
    *h_stream = s;
    *h_out_bytes = s->total;
    return 0;
}

extern "C" int uq_gzip_stream_finish(uq_gzip_stream* s, uint8_t* d_out, uint64_t out_bytes, uint32_t* h_status, uint64_t* h_bad_offset) {
    UQ_REQUIRE(s && s->ctx && h_status && h_bad_offset && (d_out || !out_bytes), "uq_gzip_stream_finish: null argument");
    UQ_REQUIRE(out_bytes >= s->total, "uq_gzip_stream_finish: %llu output bytes < %llu", (unsigned long long)out_bytes, (unsigned long long)s->total);
    *h_status = 0; *h_bad_offset = 0;
    const double t0 = now_ms();
    UQ_TRY(check_isize(s, h_status, h_bad_offset));
    if (!*h_status) UQ_TRY(finish_device(s, d_out, h_status, h_bad_offset));
    s->info.finish_ms = now_ms() - t0;
    return 0;
}

extern "C" int uq_gzip_stream_get_info(const uq_gzip_stream* s, uq_gzip_stream_info* h_info) {
    UQ_REQUIRE(s && h_info, "uq_gzip_stream_get_info: null argument");
    *h_info = s->info;
    return 0;
}

extern "C" int uq_gzip_stream_free(uq_gzip_stream* s) {
    delete s;
    return 0;
}

extern "C" int uq_gzip_stream_host(const uint8_t* h_comp, uint64_t comp_bytes, uint64_t chunk_bytes, const uint64_t* h_starts, uint64_t nstarts,
                                   uint8_t* h_out, uint64_t capacity, uint64_t* h_out_bytes, uint32_t* h_status, uint64_t* h_bad_offset,
                                   uq_gzip_stream_info* h_info) {
    UQ_REQUIRE(h_out_bytes && h_status && h_bad_offset && (h_comp || !comp_bytes) && (h_out || !capacity), "uq_gzip_stream_host: null argument");
    *h_out_bytes = 0; *h_status = 0; *h_bad_offset = 0;
    uq_gzip_stream s;
    s.comp = h_comp; s.n = comp_bytes;
    UQ_TRY(begin_common(&s, chunk_bytes, h_starts, nstarts, h_status, h_bad_offset));
    if (*h_status) return 0;
    *h_out_bytes = s.total;
    if (s.total <= capacity) {
        UQ_TRY(check_isize(&s, h_status, h_bad_offset));
        if (!*h_status) UQ_TRY(finish_host(&s, h_out, h_status, h_bad_offset));
    }
    if (h_info) *h_info = s.info;
    return 0;
}
