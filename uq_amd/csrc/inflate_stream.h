// inflate_stream.h -- gzip files that are not BGZF (one member, or members without a BSIZE field) inflated in parallel chunks: the
// speculative scheme of rapidgzip (Knespel and Brunst, 2023).  The compressed bytes are cut into chunks; in each chunk a finder looks for a
// bit offset where a deflate *unit* plausibly starts; every chunk is decoded from its offset at the same time, back-references into the
// unknown 32 KiB before the chunk coming out as *markers*; the chain of chunk ends and starts is checked (that is where correctness comes
// from); the markers are resolved once the predecessors' output is known; CRC-32 and ISIZE of every member are checked at the end.
// Shared by the GPU kernels (inflate_stream.hip, one wave per chunk) and the host entry (one "lane"); plain g++ compiles this header.
// What a deflate block is made of (bit reader, code tables and their rules, stored header) is inflate_core.h's, the same code as the
// member decoder's; this header owns the finder, the chunk's output (ring, slot) and the loop over units, blocks and symbols.
//
// Units and their canonical positions (one per unit, so that the chain check is an exact equality of (position, kind)):
//   UQ_GZS_MEMBER        a gzip member header: 8 x the byte offset of its 1f 8b;
//   UQ_GZS_UNCOMPRESSED  a stored block that is not the member's last: 8 x the byte offset of its LEN field (the header's bit position is
//                        ambiguous by the padding; a stored start always decodes with BFINAL = 0, so a final stored block is never a unit);
//   UQ_GZS_DYNAMIC       a dynamic-Huffman block: the bit offset of its 3-bit header.
//   Fixed-Huffman blocks are never searched for (too many false positives) and never end a chunk.
// A position is packed with its kind as (position << 2) | kind.
//
// The chunk decoder's output is a sequence of symbols: 0..255 bytes, 256 + w a marker for byte w of the chunk's window (the 32 KiB of the
// member's output before the chunk, w = 0 the oldest).  It keeps the last 32 768 symbols in a ring (LDS on the device) whose entries start as
// the markers 256 + w, so that a distance reaching before the chunk reads a marker with no special case, and flushes the ring to the chunk's
// slot in granules of 4 096 symbols.  The slot holds symbols [0, split) as u16 and symbols [split, len) as bytes at slot + split + i: once
// the ring holds no marker and the chunk has 32 KiB of output, no marker can follow, and the chunk switches to bytes (rapidgzip's switch).
// A chunk that starts at a member header knows its window (empty): split = 0 from the start.  The member records (one per member that ends
// inside the chunk) are stored from the slot's end downwards.  A slot that is too small ends the chunk in UQ_GZS_OVERFLOW: a normal outcome,
// the driver decodes it again with a larger slot.
//
// Safety contract (as inflate_core.h's; every input is hostile): reads go through Src::word() (zero past the data); every bit consumed is
// checked against the data's length; slot writes are checked against the slot's capacity before they happen; distances are checked against
// the member's output; every loop consumes input bits or is bounded by the data's length.
#pragma once
#include "inflate_core.h"

#define UQ_GZS_RING 32768u                      // the window
#define UQ_GZS_GRANULE 4096u                    // symbols per flush of the ring
#define UQ_GZS_NONE (~0ull)
#define UQ_GZS_MEMBER_REC 32u                   // bytes per member record in a slot

enum { UQ_GZS_MEMBER = 0, UQ_GZS_UNCOMPRESSED = 1, UQ_GZS_DYNAMIC = 2, UQ_GZS_END = 3 };

// statuses beyond inflate_core.h's UQ_INF_*
enum {
    UQ_GZS_BAD_HEADER = 13,      // bytes where a gzip member header must be (after a trailer) that are not one: no magic, not deflate,
                                 // reserved flags, a truncated header, a header CRC mismatch
    UQ_GZS_OVERFLOW = 14,        // the chunk's slot is too small (not an error: decoded again with a larger one)
    UQ_GZS_TOO_FAR_BACK = 15,    // a marker that points before the start of its member
};

// One chunk: the driver fills start / stop / slot / cap, the decoder the rest.
struct UqGzsChunk {
    uint64_t start;              // (canonical position << 2) | kind where decoding starts
    uint64_t stop;               // the next chunk's start position (bits; UQ_GZS_NONE: to the end of the data)
    uint64_t slot;               // the slot's address (device or host memory), 16-byte aligned
    uint64_t cap;                // slot bytes, a multiple of 32
    uint64_t end;                // (position << 2) | kind of the first unit at or past `stop`, or (8 n << 2) | UQ_GZS_END
    uint64_t len;                // output symbols
    uint64_t split;              // symbols [0, split) are u16 in the slot, the rest bytes
    uint64_t err_byte;           // where a status other than 0 was found (byte offset in the data; UQ_GZS_OVERFLOW: how far it got)
    uint32_t status;
    uint32_t nmem;               // member records in the slot
    uint32_t markers;            // 1: some symbol below split may be a marker
    uint32_t reserved;
};

// A member that ends inside a chunk (at slot + cap - 32 (k + 1) for the chunk's k-th one)
struct UqGzsMember {
    uint64_t out_pos;            // output symbols of the chunk before the member's end
    uint64_t trailer;            // byte offset of the member's trailer in the data
    uint32_t crc32, isize;
    uint64_t reserved;
};

// 64 bits of the data from bit offset `bit` (zero past the end)
template <class Src>
UQ_INF_HD uint64_t uq_gzs_bits64(Src& s, uint64_t bit) {
    const uint64_t b = bit >> 3;
    const uint32_t sh = (uint32_t)(bit & 7);
    const uint64_t lo = (uint64_t)s.word(b) | ((uint64_t)s.word(b + 4) << 32);
    return sh ? (lo >> sh) | ((uint64_t)s.word(b + 8) << (64 - sh)) : lo;
}

// ---- the start finder.  Cheap tests first: the member magic, a stored block's LEN / NLEN, a dynamic header's BTYPE, counts and precode
// (bits [bit, bit + 74)).  Returns a mask: 1 member, 2 stored, 4 a dynamic candidate (for uq_gzs_probe_dynamic).
template <class Src>
UQ_INF_HD uint32_t uq_gzs_probe_cheap(Src& s, uint64_t n, uint64_t bit) {
    uint32_t m = 0;
    if (bit >= 8 * n) return 0;
    if ((bit & 7) == 0) {
        const uint64_t b = bit >> 3;
        const uint32_t w = s.word(b);
        if (n - b >= 18 && (w & 0xFFFFFFu) == 0x088b1fu && !(w >> 24 & 0xE0)) m |= 1;
        // stored: LEN == ~NLEN, the block inside the data, the three bits before it zero (a non-final stored header, or zlib's zero padding)
        if (b >= 1 && n - b >= 4 && (w & 0xFFFF) == (~w >> 16 & 0xFFFF) && n - b - 4 >= (w & 0xFFFF) && !((s.word(b - 1) >> 5) & 7)) m |= 2;
    }
    const uint64_t v = uq_gzs_bits64(s, bit);
    if ((v >> 1 & 3) == 2 && (v >> 3 & 31) <= 29 && (v >> 8 & 31) <= 29) {
        const int ncode = (int)(v >> 13 & 15) + 4;
        if (uq_inf_precode_ok(uq_gzs_bits64(s, bit + 17), ncode)) m |= 4;
    }
    return m;
}

// Per-lane scratch of the full dynamic test
struct UqGzsProbe {
    uint8_t lens[320];
    uint8_t sorted[19];
    uint8_t clen[19];
    uint16_t count[16];
};

// uq_inf_kraft on lens[0, n)
UQ_INF_HD bool uq_gzs_kraft(const uint8_t* lens, int n, uint16_t* count) {
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int i = 0; i < n; ++i) count[lens[i]]++;
    return uq_inf_kraft(count);
}

// The full dynamic header at `bit`: the code lengths decode without a bad repeat, the literal/length and distance codes are valid, the
// end-of-block code is present.  One lane's work (the lanes of a wave test different offsets).
template <class Src>
UQ_INF_HD bool uq_gzs_probe_dynamic(Src& s, uint64_t n, uint64_t bit, UqGzsProbe* p) {
    const uint64_t v = uq_gzs_bits64(s, bit);
    const int nlit = (int)(v >> 3 & 31) + 257, ndist = (int)(v >> 8 & 31) + 1, ncode = (int)(v >> 13 & 15) + 4;
    const uint64_t pc = uq_gzs_bits64(s, bit + 17);
    for (int i = 0; i < 19; ++i) p->clen[i] = 0;
    for (int i = 0; i < ncode; ++i) p->clen[uq_inf_order((uint32_t)i)] = (uint8_t)(pc >> (3 * i) & 7);
    for (int l = 0; l < 8; ++l) p->count[l] = 0;
    for (int i = 0; i < 19; ++i) p->count[p->clen[i]]++;
    int offs[8];
    offs[1] = 0;
    for (int l = 1; l < 7; ++l) offs[l + 1] = offs[l] + p->count[l];
    for (int i = 0; i < 19; ++i) if (p->clen[i]) p->sorted[offs[p->clen[i]]++] = (uint8_t)i;
    uint64_t at = bit + 17 + 3 * (uint64_t)ncode;
    int k = 0, prev = -1;
    while (k < nlit + ndist) {
        if (at + 16 > 8 * n) return false;
        uint64_t w = uq_gzs_bits64(s, at);
        int code = 0, first = 0, index = 0, sym = -1, used = 0;
        for (int l = 1; l < 8; ++l) {
            code |= (int)(w >> (l - 1) & 1);
            const int c = p->count[l];
            if (code - c < first) { sym = p->sorted[index + (code - first)]; used = l; break; }
            index += c; first += c; first <<= 1; code <<= 1;
        }
        if (sym < 0) return false;
        w >>= used;
        int val = 0, rep = 1;
        if (sym < 16) { val = sym; prev = sym; }
        else if (sym == 16) { if (prev < 0) return false; val = prev; rep = 3 + (int)(w & 3); used += 2; }
        else if (sym == 17) { rep = 3 + (int)(w & 7); used += 3; prev = 0; }
        else { rep = 11 + (int)(w & 127); used += 7; prev = 0; }
        if (k + rep > nlit + ndist) return false;
        for (int r = 0; r < rep; ++r) p->lens[k + r] = (uint8_t)val;
        k += rep;
        at += (uint64_t)used;
    }
    if (p->lens[256] == 0) return false;
    return uq_gzs_kraft(p->lens, nlit, p->count) && uq_gzs_kraft(p->lens + nlit, ndist, p->count);
}

// The first unit at or after bit `lo` and before `hi` (packed (position << 2) | kind), or UQ_GZS_NONE.  The host's finder; the kernel
// runs the same tests, a wave's lanes on consecutive offsets.
template <class Src>
UQ_INF_HD uint64_t uq_gzs_find(Src& s, uint64_t n, uint64_t lo, uint64_t hi, UqGzsProbe* p) {
    for (uint64_t b = lo; b < hi && b < 8 * n; ++b) {
        const uint32_t m = uq_gzs_probe_cheap(s, n, b);
        if (m & 1) return b << 2 | UQ_GZS_MEMBER;
        if (m & 2) return b << 2 | UQ_GZS_UNCOMPRESSED;
        if ((m & 4) && uq_gzs_probe_dynamic(s, n, b, p)) return b << 2 | UQ_GZS_DYNAMIC;
    }
    return UQ_GZS_NONE;
}

// ---- a gzip member header at byte o (RFC 1952; FEXTRA skipped, FNAME / FCOMMENT up to their zero, FHCRC checked).  *data = its
// first deflate byte.
template <class Src>
UQ_INF_HD int uq_gzs_member_header(Src& s, uint64_t n, uint64_t o, const uint32_t* crctab, uint64_t* data) {
    if (o > n || n - o < 10) return UQ_GZS_BAD_HEADER;
    const uint32_t w = s.word(o);
    if ((w & 0xFFFFFFu) != 0x088b1fu) return UQ_GZS_BAD_HEADER;
    const uint32_t flg = w >> 24;
    if (flg & 0xE0) return UQ_GZS_BAD_HEADER;
    uint64_t p = o + 10;
    if (flg & 4) {
        if (n - p < 2) return UQ_GZS_BAD_HEADER;
        const uint64_t xlen = s.word(p) & 0xFFFF;
        p += 2;
        if (n - p < xlen) return UQ_GZS_BAD_HEADER;
        p += xlen;
    }
    for (uint32_t f = 8; f <= 16; f <<= 1) {
        if (!(flg & f)) continue;
        for (;;) {                                                      // bounded by the data
            if (p >= n) return UQ_GZS_BAD_HEADER;
            if ((s.word(p++) & 0xFF) == 0) break;
        }
    }
    if (flg & 2) {
        if (n - p < 2) return UQ_GZS_BAD_HEADER;
        uint32_t c = 0xFFFFFFFFu;
        for (uint64_t q = o; q < p; ++q) c = crctab[(c ^ s.word(q)) & 0xFF] ^ (c >> 8);
        if (((c ^ 0xFFFFFFFFu) & 0xFFFF) != (s.word(p) & 0xFFFF)) return UQ_GZS_BAD_HEADER;
        p += 2;
    }
    *data = p;
    return UQ_INF_OK;
}

// ---- the chunk's output: ring, flush, slot layout.  Env supplies the lanes' primitives:
//   Env::order()                   the ring writes of all lanes visible to all lanes (a no-op on the host)
//   Env::any(bool)                 true on every lane when it is true on some lane
//   Env::store16(dst, const uint32_t w[4])   one 16-byte store (dst 16-byte aligned)
template <class Env>
struct UqGzsOut {
    uint16_t* ring;
    uint8_t* slot;
    uint64_t cap, flushed, split, lastm;
    uint32_t nmem, lane, nlanes;
    bool switched, markers;
    Env& env;

    UQ_INF_HD UqGzsOut(uint16_t* r, uint8_t* s, uint64_t c, bool member_start, uint32_t l, uint32_t nl, Env& e)
        : ring(r), slot(s), cap(c), flushed(0), split(0), lastm(0), nmem(0), lane(l), nlanes(nl), switched(member_start), markers(false), env(e) {
        for (uint32_t i = lane; i < UQ_GZS_RING; i += nlanes) ring[i] = (uint16_t)(256 + i);
        env.order();
    }
    // slot bytes that symbols [0, e) take
    UQ_INF_HD uint64_t need(uint64_t e) const { return switched ? split + e : 2 * e; }
    UQ_INF_HD bool fits(uint64_t e, uint32_t nm) const { return need(e) <= cap && cap - need(e) >= (uint64_t)UQ_GZS_MEMBER_REC * nm; }

    // symbols [flushed, e) (e <= pos: written) to the slot.  Before it, the switch to bytes when the ring holds no marker.
    UQ_INF_HD void flush(uint64_t e, uint64_t pos) {
        if (!switched && pos >= UQ_GZS_RING && lastm + UQ_GZS_RING <= pos) {
            switched = true;
            const uint64_t r = (lastm + 15) & ~15ull;
            split = r > flushed ? r : flushed;
        }
        const uint64_t f = flushed;
        const uint64_t ng = (e - f + 15) / 16;
        for (uint64_t g = lane; g < ng; g += nlanes) {
            const uint64_t a = f + 16 * g;
            const uint64_t z = a + 16 < e ? a + 16 : e;
            if (switched && a >= split) {
                if (z - a == 16) {
                    uint32_t w[4];
                    for (int q = 0; q < 4; ++q) {
                        uint32_t x = 0;
                        for (int k = 0; k < 4; ++k) x |= (uint32_t)(ring[(a + 4 * q + k) & (UQ_GZS_RING - 1)] & 0xFF) << (8 * k);
                        w[q] = x;
                    }
                    env.store16(slot + split + a, w);
                } else {
                    for (uint64_t i = a; i < z; ++i) slot[split + i] = (uint8_t)ring[i & (UQ_GZS_RING - 1)];
                }
            } else {
                if (z - a == 16) {
                    for (int h = 0; h < 2; ++h) {
                        uint32_t w[4];
                        for (int q = 0; q < 4; ++q) {
                            const uint64_t i = a + 8 * h + 2 * q;
                            w[q] = (uint32_t)ring[i & (UQ_GZS_RING - 1)] | ((uint32_t)ring[(i + 1) & (UQ_GZS_RING - 1)] << 16);
                        }
                        env.store16(slot + 2 * a + 16 * h, w);
                    }
                } else {
                    for (uint64_t i = a; i < z; ++i) {
                        const uint16_t v = ring[i & (UQ_GZS_RING - 1)];
                        slot[2 * i] = (uint8_t)v;
                        slot[2 * i + 1] = (uint8_t)(v >> 8);
                    }
                }
            }
        }
        flushed = e;
    }
    // room for symbols [pos, pos + len) (len <= UQ_GZS_GRANULE): flush what the ring is about to overwrite; false: the slot is too small
    UQ_INF_HD bool reserve(uint64_t pos, uint32_t len) {
        while (pos + len > flushed + UQ_GZS_RING) flush(flushed + UQ_GZS_GRANULE, pos);
        return fits(pos + len, nmem);
    }
    UQ_INF_HD void put(uint64_t pos, uint32_t b) {
        if (lane == 0) ring[pos & (UQ_GZS_RING - 1)] = (uint16_t)b;
        env.order();
    }
    // [pos, pos + len) from pos - dist (dist <= 32 768; before the chunk: the ring's markers)
    UQ_INF_HD void copy(uint64_t pos, uint32_t dist, uint32_t len) {
        bool mk = false;
        if (dist >= nlanes) {
            for (uint32_t i = lane; i < len; i += nlanes) {
                const uint16_t v = ring[(pos - dist + i) & (UQ_GZS_RING - 1)];
                ring[(pos + i) & (UQ_GZS_RING - 1)] = v;
                mk |= v >= 256;
            }
        } else {
            for (uint32_t i = lane; i < len; i += nlanes) {
                const uint16_t v = ring[(pos - dist + i % dist) & (UQ_GZS_RING - 1)];
                ring[(pos + i) & (UQ_GZS_RING - 1)] = v;
                mk |= v >= 256;
            }
        }
        env.order();
        if (!switched && env.any(mk)) { lastm = pos + len; markers = true; }
    }
    template <class Src>
    UQ_INF_HD void stored(uint64_t pos, Src& src, uint64_t at, uint32_t len) {
        for (uint32_t i = lane; i < len; i += nlanes) ring[(pos + i) & (UQ_GZS_RING - 1)] = (uint16_t)(src.byte(at + i));
        env.order();
    }
    UQ_INF_HD bool member_end(uint64_t pos, uint32_t crc, uint32_t isize, uint64_t trailer) {
        if (!fits(pos, nmem + 1)) return false;
        if (lane == 0) {
            UqGzsMember* m = (UqGzsMember*)(slot + cap - (uint64_t)UQ_GZS_MEMBER_REC * (nmem + 1));
            m->out_pos = pos; m->trailer = trailer; m->crc32 = crc; m->isize = isize; m->reserved = 0;
        }
        ++nmem;
        return true;
    }
};

// A stored block's body from its LEN field (the reader byte-aligned).  *pos advances.
template <class B, class Src, class Out>
UQ_INF_HD int uq_gzs_copy_block(B& br, Src& src, Out& out, uint64_t* pos) {
    uint32_t l;
    uint64_t at;
    const int st = uq_inf_stored_header(br, &l, &at);
    if (st) return st;
    for (uint32_t d = 0; d < l; d += UQ_GZS_GRANULE) {
        const uint32_t k = l - d < UQ_GZS_GRANULE ? l - d : UQ_GZS_GRANULE;
        if (!out.reserve(*pos, k)) return UQ_GZS_OVERFLOW;
        out.stored(*pos, src, at + d, k);
        *pos += k;
    }
    br.seek(at + l);
    return UQ_INF_OK;
}

// ---- one chunk: from c->start, whole units, up to the first unit whose canonical position is >= c->stop (never the first one) or the
// end of the data.  Fills c->end / len / split / status / err_byte / nmem / markers; the symbols and member records go to the slot.
template <class Src, class Env>
UQ_INF_HD void uq_gzs_chunk(Src& src, uint64_t n, UqGzsChunk* c, uint16_t* ring, UqInflateTables* t, const uint32_t* crctab,
                            uint32_t lane, uint32_t nlanes, Env& env) {
    const uint64_t start = c->start, stop = c->stop;
    uint64_t ubit = start >> 2;
    int ukind = (int)(start & 3);
    UqGzsOut<Env> out(ring, (uint8_t*)(uintptr_t)c->slot, c->cap, ukind == UQ_GZS_MEMBER, lane, nlanes, env);
    UqBits<Src, uint64_t> br(src, n);
    uint64_t pos = 0, mbase = 0, end = UQ_GZS_NONE;
    bool known = false, first = true;
    int st = UQ_INF_OK;
    uint64_t err = ubit >> 3;
    if (ukind == UQ_GZS_END || ubit > 8 * n) { st = UQ_INF_TRUNCATED; goto done; }
    for (;;) {                                                          // units: each consumes >= 1 byte of the data
        if (!first && ubit >= stop) { end = ubit << 2 | (uint64_t)ukind; break; }
        if (ukind == UQ_GZS_MEMBER) {
            uint64_t data = 0;
            err = ubit >> 3;
            st = uq_gzs_member_header(src, n, ubit >> 3, crctab, &data);
            if (st) goto done;
            known = true; mbase = pos;
            br.seek(data);
        } else if (ukind == UQ_GZS_UNCOMPRESSED) {
            br.seek(ubit >> 3);
            err = ubit >> 3;
            st = uq_gzs_copy_block(br, src, out, &pos);
            if (st) goto done;
        } else {
            br.seek_bit(ubit);
        }
        // blocks: each consumes >= 3 bits
        bool check = ukind != UQ_GZS_DYNAMIC || !first;
        first = false;
        bool final = false;
        while (!final) {
            br.refill();
            const uint64_t p = br.bit_pos();
            err = p >> 3;
            const uint32_t hdr = br.peek(3);
            const uint32_t type = hdr >> 1;
            if (check) {
                if (type == 2 && p >= stop) { end = p << 2 | UQ_GZS_DYNAMIC; goto done; }
                if (type == 0 && !(hdr & 1)) {
                    const uint64_t cpos = (p + 3 + 7) & ~7ull;
                    if (cpos >= stop) { end = cpos << 2 | UQ_GZS_UNCOMPRESSED; goto done; }
                }
            }
            check = true;
            br.drop(3);
            if (br.overrun()) { st = UQ_INF_TRUNCATED; goto done; }
            final = hdr & 1;
            if (type == 0) {
                br.align();
                st = uq_gzs_copy_block(br, src, out, &pos);
                if (st) goto done;
                continue;
            }
            if (type == 3) { st = UQ_INF_BAD_BLOCK_TYPE; goto done; }
            st = uq_inf_tables(br, type, t, lane, nlanes, env);
            if (st) goto done;
            for (;;) {                                                  // symbols: each consumes >= 1 bit
                br.refill();
                const int sym = uq_inf_decode(br, &t->hlit, t->lit, UQ_INF_LIT_BITS);
                if (br.overrun()) { st = UQ_INF_TRUNCATED; goto done; }
                if (sym < 0) { st = UQ_INF_BAD_SYMBOL; goto done; }
                if (sym < 256) {
                    if (!out.reserve(pos, 1)) { st = UQ_GZS_OVERFLOW; goto done; }
                    out.put(pos++, (uint32_t)sym);
                    continue;
                }
                if (sym == 256) break;
                const int li = sym - 257;                               // the match: uq_inflate_core has the same lines
                if (li >= 29) { st = UQ_INF_BAD_SYMBOL; goto done; }
                uint32_t length;
                if (li < 8) length = 3 + (uint32_t)li;
                else if (li == 28) length = 258;
                else { const int ex = (li >> 2) - 1; length = ((4u + (uint32_t)(li & 3)) << ex) + 3 + br.get((uint32_t)ex); }
                br.refill();
                const int ds = uq_inf_decode(br, &t->hdist, t->dist, UQ_INF_DIST_BITS);
                if (ds < 0 || ds >= 30) { st = br.overrun() ? UQ_INF_TRUNCATED : UQ_INF_BAD_SYMBOL; goto done; }
                uint32_t dist;
                if (ds < 4) dist = (uint32_t)ds + 1;
                else { const int ex = (ds >> 1) - 1; dist = ((2u + (uint32_t)(ds & 1)) << ex) + 1 + br.get((uint32_t)ex); }
                if (br.overrun()) { st = UQ_INF_TRUNCATED; goto done; }
                if (known && dist > pos - mbase) { st = UQ_INF_BAD_DISTANCE; goto done; }
                if (!out.reserve(pos, length)) { st = UQ_GZS_OVERFLOW; goto done; }
                out.copy(pos, dist, length);
                pos += length;
            }
        }
        // the member's trailer, then the next member's header or the end of the data
        br.align();
        err = br.byte_pos();
        {
            const uint32_t c0 = br.get(16), c1 = br.get(16), i0 = br.get(16), i1 = br.get(16);
            if (br.overrun()) { st = UQ_INF_TRUNCATED; goto done; }
            const uint64_t o = br.byte_pos();
            if (!out.member_end(pos, c0 | c1 << 16, i0 | i1 << 16, o - 8)) { st = UQ_GZS_OVERFLOW; goto done; }
            if (o == n) { end = (8 * n) << 2 | UQ_GZS_END; break; }
            ubit = 8 * o;
            ukind = UQ_GZS_MEMBER;
        }
    }
done:
    if (st == UQ_INF_OK) out.flush(pos, pos);
    if (st == UQ_GZS_OVERFLOW) err = br.byte_pos();                  // how far the slot lasted: the driver sizes the next one from it
    if (lane == 0) {
        c->status = (uint32_t)st;
        c->end = end;
        c->len = pos;
        c->split = out.switched ? out.split : pos;
        c->err_byte = err;
        c->nmem = out.nmem;
        c->markers = out.markers ? 1u : 0u;
    }
}
