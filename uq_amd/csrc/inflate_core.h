// inflate_core.h -- RFC 1951 (deflate) decoding, shared by the GPU kernels and the host entries (one "lane"), so that the decoder's handling of
// corrupt input can be exercised on a CPU under AddressSanitizer with the very code the GPU runs.  Plain g++ compiles this header: the
// qualifiers are guarded.  Two decoders are built from it: uq_inflate_core below (one gzip member into a buffer of known size: inflate.hip,
// one wave per member) and uq_gzs_chunk (inflate_stream.h: a chunk of a gzip file from a speculative start).  Everything a deflate block
// is made of lives here once, for both: the bit reader (UqBits), the block's code tables from its header (uq_inf_tables, with the rules a
// set of code lengths must meet: uq_inf_precode_ok, uq_inf_kraft) and a stored block's header (uq_inf_stored_header).  The two symbol loops
// stay apart: they differ in what bounds the output, in the distance rule and in where a decode may stop.  Each keeps its own copy of the
// dozen lines that turn a length symbol into (length, distance): as a shared function, in three forms, they made inflate_members_kernel
// 3 to 7 % slower on the MI355X.
//
// Safety contract (every input is hostile):
//   - the compressed bytes are read only through Src::word(), whose reads are bounded by the member's compressed length; bytes past it
//     read as zero, and the decoder stops with UQ_INF_TRUNCATED as soon as it has consumed a bit it does not own;
//   - the output is written only through Out, and only below isize: every literal, match and stored copy is checked against it first;
//   - every distance is checked against the bytes produced so far;
//   - over-subscribed code-length sets are rejected, incomplete ones too except the single one-bit code deflate allows (not for the
//     code-length code, which must be complete: zlib's rule);
//   - every loop is bounded: a block and a symbol each consume at least one bit, and consumption is checked against the bit budget.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UQ_INF_HD __host__ __device__ __forceinline__
#else
#define UQ_INF_HD inline
#endif

// per-member status words (0 = inflated, length and CRC-32 verified)
enum {
    UQ_INF_OK = 0,
    UQ_INF_TRUNCATED = 1,          // the deflate stream needs bytes past the member's compressed length
    UQ_INF_BAD_BLOCK_TYPE = 2,     // BTYPE 11
    UQ_INF_BAD_STORED_LEN = 3,     // stored block LEN != ~NLEN
    UQ_INF_BAD_CODE_LENGTHS = 4,   // over-subscribed or incomplete code-length set, or no end-of-block code
    UQ_INF_BAD_REPEAT = 5,         // code-length repeat with no previous length, or past the end of the list
    UQ_INF_BAD_SYMBOL = 6,         // a code that is not in the table, or length symbol 286/287, distance symbol 30/31
    UQ_INF_BAD_DISTANCE = 7,       // a distance reaching before the start of the member's output
    UQ_INF_OUTPUT_OVERFLOW = 8,    // more output than ISIZE
    UQ_INF_ISIZE_MISMATCH = 9,     // less output than ISIZE
    UQ_INF_CRC_MISMATCH = 10,      // CRC-32 of the output != the trailer's
    UQ_INF_BAD_COUNTS = 11,        // HLIT > 286 or HDIST > 30
    UQ_INF_TOO_LARGE = 12,         // ISIZE beyond UQ_INF_MAX_OUT, or the member outside the buffers it was given
};

#define UQ_INF_MAX_OUT 65536u      // a BGZF member's output bound; the kernel keeps it whole in LDS
#define UQ_INF_LIT_BITS 10         // primary lookup bits of the literal/length table (longer codes: slow path)
#define UQ_INF_DIST_BITS 8         // ... of the distance table
#define UQ_INF_CLEN_BITS 7         // code-length codes are at most 7 bits long: no slow path

// One Huffman code: primary table entries are (symbol << 4) | length, 0 = not a code of <= `bits` bits (a longer one, or none).
// count / sorted: the canonical description (count of codes of every length, symbols ordered by (length, value)) for the slow path.
struct UqHuff {
    uint16_t count[16];
    uint16_t offs[16];
    uint16_t sorted[288];
};

struct UqInflateTables {
    uint16_t lit[1 << UQ_INF_LIT_BITS];
    uint16_t dist[1 << UQ_INF_DIST_BITS];
    uint16_t clen[1 << UQ_INF_CLEN_BITS];
    UqHuff hlit, hdist, hclen;
    uint8_t lens[288 + 32];
};

UQ_INF_HD uint32_t uq_inf_rev(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) { r = (r << 1) | (code & 1); code >>= 1; }
    return r;
}

// The order in which a dynamic block's header sends the code-length code's lengths (RFC 1951 3.2.7)
UQ_INF_HD uint32_t uq_inf_order(uint32_t i) {
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

// The rule for a code, given its count of codes of every length 1..15: not over-subscribed, and complete unless it is at most one code of
// one bit (deflate allows that, for a block with a single distance or none)
UQ_INF_HD bool uq_inf_kraft(const uint16_t* count) {
    int left = 1, maxlen = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - count[l];
        if (left < 0) return false;
        if (count[l]) maxlen = l;
    }
    return !(left > 0 && maxlen > 1);
}

// The stricter rule for the code-length code (zlib's): complete.  v: up to 19 three-bit lengths as the header sends them, length i at bits 3i
UQ_INF_HD bool uq_inf_precode_ok(uint64_t v, int ncode) {
    int left = 1;
    for (int l = 1; l < 8; ++l) {
        int c = 0;
        for (int i = 0; i < ncode; ++i) c += (int)(((v >> (3 * i)) & 7) == (uint64_t)l);
        left = 2 * left - c;
        if (left < 0) return false;
    }
    return left == 0;
}

// Builds the canonical description of the code of n lengths into `h` and clears the primary table `tab` (1 << bits entries).  lane / nlanes:
// the work is spread over the lanes of a wave (the host passes 0 / 1).  Arrays that are indexed by data live in `h` (LDS on the device),
// never in registers; `sync()` orders one phase's writes by some lanes before the next phase's reads by others.
template <class Sync>
UQ_INF_HD int uq_inf_build(const uint8_t* lens, int n, UqHuff* h, uint16_t* tab, int bits, uint32_t lane, uint32_t nlanes, Sync& sync) {
    for (uint32_t l = lane; l < 16; l += nlanes) {
        uint32_t c = 0;
        for (int s = 0; s < n; ++s) c += (uint32_t)(lens[s] == l);
        h->count[l] = (uint16_t)(l ? c : 0);
    }
    sync.sync();
    if (!uq_inf_kraft(h->count)) return UQ_INF_BAD_CODE_LENGTHS;
    if (lane == 0) {
        uint32_t off = 0;
        for (int l = 1; l < 16; ++l) { h->offs[l] = (uint16_t)off; off += h->count[l]; }
    }
    for (uint32_t e = lane; e < (1u << bits); e += nlanes) tab[e] = 0;
    sync.sync();
    if (lane == 0)                                                      // symbols in canonical order
        for (int s = 0; s < n; ++s) {
            const int l = lens[s];
            if (l) h->sorted[h->offs[l]++] = (uint16_t)s;
        }
    sync.sync();
    return UQ_INF_OK;
}

// Second half of the build (after the sorted list is visible to every lane): the primary table entries of the codes of <= bits bits.
UQ_INF_HD void uq_inf_fill(const UqHuff* h, uint16_t* tab, int bits, uint32_t lane, uint32_t nlanes) {
    uint32_t code = 0, index = 0;
    for (int l = 1; l <= bits; ++l) {
        const uint32_t cnt = h->count[l];
        for (uint32_t j = lane; j < cnt; j += nlanes) {
            const uint32_t sym = h->sorted[index + j];
            const uint32_t r = uq_inf_rev(code + j, l);
            for (uint32_t k = r; k < (1u << bits); k += 1u << l) tab[k] = (uint16_t)((sym << 4) | (uint32_t)l);
        }
        index += cnt;
        code = (code + cnt) << 1;
    }
}

// The bit reader over Src::word(byte offset) = the 4 bytes there, little-endian, zero past the data's end.  Off is the type of a byte offset:
// 32 bits for a BGZF member (fewer registers, and the offset is made wave-uniform with one v_readfirstlane), 64 for a whole file.
template <class Src, class Off = uint32_t>
struct UqBits {
    Src& src;
    uint64_t buf;
    uint32_t cnt;       // valid bits in buf
    Off pos;            // next byte offset to load
    Off len;            // compressed length in bytes
    UQ_INF_HD UqBits(Src& s, Off n) : src(s), buf(0), cnt(0), pos(0), len(n) {}
    UQ_INF_HD void refill() {
        if (cnt <= 32) { buf |= (uint64_t)src.word(pos) << cnt; pos += 4; cnt += 32; }
    }
    UQ_INF_HD uint32_t peek(uint32_t n) const { return (uint32_t)buf & ((1u << n) - 1); }
    UQ_INF_HD void drop(uint32_t n) { buf >>= n; cnt -= n; }
    UQ_INF_HD uint32_t get(uint32_t n) { refill(); uint32_t v = peek(n); drop(n); return v; }   // n <= 16
    UQ_INF_HD uint64_t bit_pos() const { return 8ull * pos - cnt; }                              // of the next unread bit
    UQ_INF_HD bool overrun() const { return bit_pos() > 8ull * len; }
    UQ_INF_HD Off byte_pos() const { return pos - cnt / 8; }                                     // after align(): the next unread byte
    UQ_INF_HD void align() { drop(cnt & 7); }
    UQ_INF_HD void seek(Off p) { buf = 0; cnt = 0; pos = p; }
    UQ_INF_HD void seek_bit(uint64_t b) { seek((Off)(b >> 3)); refill(); drop((uint32_t)(b & 7)); }
};

// One symbol of code (h, tab): the primary table, or the canonical walk for codes longer than `bits`.  Needs >= 15 bits in the buffer.
// Returns the symbol, or -1 for a bit pattern that is no code.
template <class B>
UQ_INF_HD int uq_inf_decode(B& br, const UqHuff* h, const uint16_t* tab, int bits) {
    const uint32_t e = tab[br.peek(bits)];
    if (e & 15) { br.drop(e & 15); return (int)(e >> 4); }
    const uint32_t v = br.peek(15);
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (int)((v >> (l - 1)) & 1);
        const int count = h->count[l];
        if (code - count < first) { br.drop((uint32_t)l); return h->sorted[index + (code - first)]; }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

UQ_INF_HD void uq_inf_fixed_lens(uint8_t* lens, uint32_t lane, uint32_t nlanes) {
    for (uint32_t s = lane; s < 288 + 32; s += nlanes)
        lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
}

// One block's code tables, fixed (type 1) or dynamic (type 2, from the header that follows BTYPE): t->lit / hlit and t->dist / hdist ready
// for uq_inf_decode.  Sync::sync() orders one phase's table writes by some lanes before the next phase's reads by others.  The rules are
// zlib's: the code-length code complete, the other two as uq_inf_kraft, an end-of-block code present.
template <class B, class Sync>
UQ_INF_HD int uq_inf_tables(B& br, uint32_t type, UqInflateTables* t, uint32_t lane, uint32_t nlanes, Sync& sync) {
    int nlit = 288, ndist = 32;
    if (type == 1) {
        uq_inf_fixed_lens(t->lens, lane, nlanes);
        sync.sync();
    } else {
        nlit = (int)br.get(5) + 257;
        ndist = (int)br.get(5) + 1;
        const int ncode = (int)br.get(4) + 4;
        if (nlit > 286 || ndist > 30) return UQ_INF_BAD_COUNTS;
        // the code-length code's lengths in lens[0, 19)
        for (uint32_t i = lane; i < 19; i += nlanes) t->lens[i] = 0;
        sync.sync();
        uint64_t pc = 0;
        for (int i = 0; i < ncode; ++i) {
            const uint32_t v = br.get(3);
            pc |= (uint64_t)v << (3 * i);
            if (lane == 0) t->lens[uq_inf_order((uint32_t)i)] = (uint8_t)v;
        }
        if (br.overrun()) return UQ_INF_TRUNCATED;
        if (!uq_inf_precode_ok(pc, ncode)) return UQ_INF_BAD_CODE_LENGTHS;
        sync.sync();
        int st = uq_inf_build(t->lens, 19, &t->hclen, t->clen, UQ_INF_CLEN_BITS, lane, nlanes, sync);
        if (st) return st;
        uq_inf_fill(&t->hclen, t->clen, UQ_INF_CLEN_BITS, lane, nlanes);
        sync.sync();
        // nlit + ndist code lengths; every iteration consumes >= 1 bit
        int n = 0, prev = -1;
        while (n < nlit + ndist) {
            br.refill();
            const int sym = uq_inf_decode(br, &t->hclen, t->clen, UQ_INF_CLEN_BITS);
            if (br.overrun()) return UQ_INF_TRUNCATED;
            if (sym < 0) return UQ_INF_BAD_SYMBOL;
            int val = 0, rep = 1;
            if (sym < 16) { val = sym; prev = sym; }
            else if (sym == 16) { if (prev < 0) return UQ_INF_BAD_REPEAT; val = prev; rep = 3 + (int)br.get(2); }
            else if (sym == 17) { rep = 3 + (int)br.get(3); }
            else { rep = 11 + (int)br.get(7); }
            if (sym == 17 || sym == 18) prev = 0;
            if (n + rep > nlit + ndist) return UQ_INF_BAD_REPEAT;
            if (lane == 0) for (int k = 0; k < rep; ++k) t->lens[n + k] = (uint8_t)val;
            n += rep;
        }
        if (br.overrun()) return UQ_INF_TRUNCATED;
        sync.sync();
        // the distance lengths go to lens[288...]: the fixed layout, so that one fill serves both forms
        if (lane == 0) for (int k = ndist - 1; k >= 0; --k) t->lens[288 + k] = t->lens[nlit + k];
        sync.sync();
        if (t->lens[256] == 0) return UQ_INF_BAD_CODE_LENGTHS;           // no end-of-block code
    }
    int st = uq_inf_build(t->lens, nlit, &t->hlit, t->lit, UQ_INF_LIT_BITS, lane, nlanes, sync);
    if (st) return st;
    st = uq_inf_build(t->lens + 288, ndist, &t->hdist, t->dist, UQ_INF_DIST_BITS, lane, nlanes, sync);
    if (st) return st;
    uq_inf_fill(&t->hlit, t->lit, UQ_INF_LIT_BITS, lane, nlanes);
    uq_inf_fill(&t->hdist, t->dist, UQ_INF_DIST_BITS, lane, nlanes);
    sync.sync();
    return UQ_INF_OK;
}

// A stored block's LEN / NLEN (the reader byte-aligned at LEN): *len = LEN, *at = the byte offset of the block's first byte.  The whole block
// lies inside the data.
template <class Src, class Off>
UQ_INF_HD int uq_inf_stored_header(UqBits<Src, Off>& br, uint32_t* len, Off* at) {
    const uint32_t l = br.get(16), nl = br.get(16);
    if (br.overrun()) return UQ_INF_TRUNCATED;
    if (l != (~nl & 0xFFFFu)) return UQ_INF_BAD_STORED_LEN;
    *len = l;
    *at = br.byte_pos();
    if ((uint64_t)*at + l > br.len) return UQ_INF_TRUNCATED;
    return UQ_INF_OK;
}

// Inflates one raw deflate stream of `clen` bytes into exactly `isize` bytes.
//   Out::put(pos, byte)               one literal at output offset pos (< isize)
//   Out::copy(pos, dist, len)         bytes [pos, pos + len) from pos - dist (dist <= pos, pos + len <= isize; may overlap)
//   Out::stored(pos, src_off, len)    `len` compressed bytes from src_off (src_off + len <= clen) to [pos, pos + len)
//   Out::sync()                       orders the lanes' table writes before the reads that follow
template <class Src, class Out>
UQ_INF_HD int uq_inflate_core(Src& src, uint32_t clen, Out& out, uint32_t isize, UqInflateTables* t, uint32_t lane, uint32_t nlanes) {
    UqBits<Src> br(src, clen);
    uint32_t pos = 0;
    for (;;) {                                                          // blocks: each header consumes 3 bits, checked against the budget
        const uint32_t hdr = br.get(3);
        if (br.overrun()) return UQ_INF_TRUNCATED;
        const uint32_t type = hdr >> 1;
        if (type == 0) {
            br.align();
            uint32_t l, at;
            const int st = uq_inf_stored_header(br, &l, &at);
            if (st) return st;
            if ((uint64_t)pos + l > isize) return UQ_INF_OUTPUT_OVERFLOW;
            out.stored(pos, at, l);
            pos += l;
            br.seek(at + l);
        } else if (type == 3) {
            return UQ_INF_BAD_BLOCK_TYPE;
        } else {
            int st = uq_inf_tables(br, type, t, lane, nlanes, out);
            if (st) return st;
            for (;;) {                                                  // symbols: each consumes >= 1 bit, checked against the budget
                br.refill();
                const int sym = uq_inf_decode(br, &t->hlit, t->lit, UQ_INF_LIT_BITS);
                if (br.overrun()) return UQ_INF_TRUNCATED;
                if (sym < 0) return UQ_INF_BAD_SYMBOL;
                if (sym < 256) {
                    if (pos >= isize) return UQ_INF_OUTPUT_OVERFLOW;
                    out.put(pos++, (uint8_t)sym);
                    continue;
                }
                if (sym == 256) break;
                const int li = sym - 257;                               // the match: uq_gzs_chunk has the same lines (see the file head)
                if (li >= 29) return UQ_INF_BAD_SYMBOL;
                uint32_t length;
                if (li < 8) length = 3 + (uint32_t)li;
                else if (li == 28) length = 258;
                else { const int ex = (li >> 2) - 1; length = ((4u + (uint32_t)(li & 3)) << ex) + 3 + br.get((uint32_t)ex); }
                br.refill();
                const int ds = uq_inf_decode(br, &t->hdist, t->dist, UQ_INF_DIST_BITS);
                if (ds < 0 || ds >= 30) { if (br.overrun()) return UQ_INF_TRUNCATED; return UQ_INF_BAD_SYMBOL; }
                uint32_t dist;
                if (ds < 4) dist = (uint32_t)ds + 1;
                else { const int ex = (ds >> 1) - 1; dist = ((2u + (uint32_t)(ds & 1)) << ex) + 1 + br.get((uint32_t)ex); }
                if (br.overrun()) return UQ_INF_TRUNCATED;
                if (dist > pos) return UQ_INF_BAD_DISTANCE;
                if ((uint64_t)pos + length > isize) return UQ_INF_OUTPUT_OVERFLOW;
                out.copy(pos, dist, length);
                pos += length;
            }
        }
        if (hdr & 1) break;                                             // BFINAL
    }
    if (pos != isize) return UQ_INF_ISIZE_MISMATCH;
    return UQ_INF_OK;
}

// ---- CRC-32 (gzip's, reflected polynomial 0xEDB88320) and its shift operators: crc(A || B) = (crc0(A) * x^(8|B|)) ^ crc0(B) for the
// zero-initialised, un-inverted CRC crc0, which lets the lanes of a wave each take a segment and combine the results.
#define UQ_CRC_POLY 0xEDB88320u

UQ_INF_HD uint32_t uq_crc_table_entry(uint32_t b) {
    uint32_t c = b;
    for (int k = 0; k < 8; ++k) c = c & 1 ? (c >> 1) ^ UQ_CRC_POLY : c >> 1;
    return c;
}

// a * b modulo the polynomial (bit 31 = x^0)
UQ_INF_HD uint32_t uq_crc_multmodp(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = b & 1 ? (b >> 1) ^ UQ_CRC_POLY : b >> 1;
    }
    return p;
}

// x2n[k] = x^(2^k) modulo the polynomial, k < 32
UQ_INF_HD void uq_crc_x2n_init(uint32_t* x2n) {
    uint32_t p = 0x40000000u;                                           // x^1
    for (int k = 0; k < 32; ++k) { x2n[k] = p; p = uq_crc_multmodp(p, p); }
}

// x^(8 n) modulo the polynomial: the operator that moves a CRC over n zero bytes
UQ_INF_HD uint32_t uq_crc_shift_op(const uint32_t* x2n, uint64_t n) {
    uint32_t p = 0x80000000u;                                           // x^0
    for (int k = 3; n && k < 64; n >>= 1, ++k)
        if (n & 1) p = uq_crc_multmodp(x2n[k & 31], p);
    return p;
}

// crc0 (zero start, no final inversion) of bytes through the byte table
UQ_INF_HD uint32_t uq_crc0_bytes(const uint32_t* table, uint32_t c, const uint8_t* p, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return c;
}

// gzip's CRC-32 of an n-byte message from its crc0: the 0xFFFFFFFF start carried over n bytes, and the final inversion
UQ_INF_HD uint32_t uq_crc_finish(const uint32_t* x2n, uint32_t crc0, uint64_t n) {
    return crc0 ^ uq_crc_multmodp(uq_crc_shift_op(x2n, n), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
}
