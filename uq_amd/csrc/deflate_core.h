// deflate_core.h -- RFC 1951 compression of one BGZF block into one complete gzip member, shared by the GPU kernel (deflate.hip, one
// workgroup per block) and the host entry uq_bgzf_compress_block_host (one "thread"), so that the device's bytes can be compared with a
// CPU build of the very same code, and the code run under AddressSanitizer.  Plain g++ compiles this header.
//
// The member's bytes depend on the input bytes only: every phase is defined on fixed position ranges (UQ_DEF_ROUND, UQ_DEF_SUB), never on
// the thread count, and the only LDS atomics are commutative (max, add, xor).
//
//   1. CRC-32 of the block: per-thread segments, combined with the shift operators of inflate_core.h.
//   2. Matches, round by round (UQ_DEF_ROUND positions): a position hashes its 4 bytes and looks up `head`, which holds the latest
//      position with that hash *before the round*; the candidate is compared byte by byte (length 3..258, distance <= 32 768).  After the
//      round, `head` takes the round's positions by atomic max.  Each position's match length goes to LDS (one byte, `len`), its
//      distance to the environment's workspace (dist_put / dist_get: HBM on the device).
//   3. Greedy parse: the block is cut into sub-segments of UQ_DEF_SUB positions; pointer jumping over a window of sub-segments gives,
//      for every position, the first token start at or past the end of its sub-segment, and one thread chains those into the first token
//      start of every sub-segment (`entry`).  After that, each sub-segment's tokens are a walk of at most UQ_DEF_SUB steps.
//   4. Walk 1: literal/length and distance histograms (LDS atomic adds).  One dynamic-Huffman block: code lengths limited to 15 bits
//      (7 for the code-length code) by clamping small weights and rebuilding, the code-length sequence run-length coded with 16/17/18.
//   5. Walk 2: the bits of every sub-segment; an exclusive scan gives its bit offset.  A stored block is written instead when it is smaller.
//   6. Walk 3: every range of bits (the staged header, each sub-segment, the end-of-block code and the trailer) is written by one thread:
//      words it covers whole are stored, the partial words at its ends are OR-ed in (the output starts zeroed, and OR is commutative).
//
// Level 2 (kLevel = 2: UqDeflateLds2 / UqDeflateSizeLds2, uq_deflate_block_l / uq_deflate_block_size_l) changes phases 2 and 3 only:
//   2. Up to five candidates per position, the longest wins, a tie takes the nearer: the two positions of a packed `head` word
//      ((newest + 1) << 16 | (older + 1): after a round, atomic max with ((p + 1) << 16) | the newest from before the round, which every
//      position noted in `prev` before the barrier), the fixed distances 1 and 2 (runs, from the block's first bytes on), and the
//      distance of the last match of the round before (`rep`, an atomic max of (position << 16 | distance - 1): a copy longer than a
//      round goes on where the hash table has long been overwritten).
//   3. Lazy parse: a position is a literal when it has no match, or when its match is shorter than UQ_DEF_LAZY_MAX and the match at the
//      next position is longer.  The decision reads len[p] and len[p + 1] only (uq_def_tok), so the pointer jumping and the three walks
//      keep their shape.
//
// Safety: reads of the block stay below n (n <= UQ_DEF_MAX_IN); the member's size is known before anything is written and is checked
// against the capacity (UQ_DEF_NO_SPACE otherwise); every loop has a bound that does not depend on the data.
#pragma once
#include <stdint.h>
#include "inflate_core.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UQ_DEF_HD __host__ __device__ __forceinline__
#else
#define UQ_DEF_HD inline
#endif

enum {
    UQ_DEF_OK = 0,
    UQ_DEF_NO_SPACE = 1,           // the member is larger than the output capacity given
    UQ_DEF_TOO_LARGE = 2,          // more than UQ_DEF_MAX_IN input bytes
};

#define UQ_DEF_MAX_IN 65280u       // bgzip's block size
#define UQ_DEF_MAX_MEMBER 65311u   // 18 header + 5 stored-block header + 65 280 + 8 trailer
#define UQ_DEF_ROUND 512u          // positions that look up `head` together (and cannot see each other)
#define UQ_DEF_HASH_BITS 12
#define UQ_DEF_SUB 128u            // positions of a parse sub-segment
#define UQ_DEF_NSUB ((UQ_DEF_MAX_IN + UQ_DEF_SUB - 1) / UQ_DEF_SUB)
#define UQ_DEF_WIN 8192u           // positions of a pointer-jumping window (u16 entries in the head table's space)
#define UQ_DEF_HDR_WORDS 160       // gzip header + dynamic block header: 144 + 17 + 57 + 316 * 14 bits < 160 words
#define UQ_DEF_NONE 0xFFFFu
#define UQ_DEF_LAZY_MAX 32u        // level 2: a match of at least this many bytes is taken without looking at the next position

struct UqDefHuffScratch {
    uint16_t sorted[288];          // symbols with a weight, by (weight, symbol)
    uint32_t weight[576];          // leaves 0..m-1 (sorted order), internal nodes m..2m-2
    uint16_t parent[576];
    uint8_t depth[576];
    uint32_t done;
};

struct UqDeflateLds {
    uint8_t in[UQ_DEF_MAX_IN + 16];
    uint8_t len[UQ_DEF_MAX_IN];    // 0 = literal; v in 1..254: a match of v + 2 bytes; 255: 258 bytes
    union {
        uint32_t head[1u << UQ_DEF_HASH_BITS];          // position + 1, 0 = none
        uint16_t jmp[UQ_DEF_WIN];                       // parse: first token start past the sub-segment, relative to the window
        UqDefHuffScratch h;
    } u;
    uint32_t lfreq[288], dfreq[32], cfreq[20];
    uint8_t llen[288], dlen[32], clen[20];
    uint16_t lcode[288], dcode[32], ccode[20];
    uint16_t rle[320];             // code-length symbols (0..18); the extra bits of 16/17/18 in rlex
    uint8_t rlex[320];
    uint16_t entry[UQ_DEF_NSUB];   // first token start of each sub-segment, UQ_DEF_NONE = none
    uint32_t bits[UQ_DEF_NSUB + 2];// per range: bit count, then its first bit
    uint32_t hdr[UQ_DEF_HDR_WORDS];
    uint32_t crctab[256];
    uint32_t crc0, nrle, hlit, hdist, hclen, hdr_bits, member_bytes, stored;
};

// what the size-only path (uq_deflate_block_size) needs of the above: no codes, no extra bits of the run-length code, no bit offsets, no
// staged header, no CRC
struct UqDeflateSizeLds {
    uint8_t in[UQ_DEF_MAX_IN + 16];
    uint8_t len[UQ_DEF_MAX_IN];
    union {
        uint32_t head[1u << UQ_DEF_HASH_BITS];
        uint16_t jmp[UQ_DEF_WIN];
        UqDefHuffScratch h;
    } u;
    uint32_t lfreq[288], dfreq[32], cfreq[20];
    uint8_t llen[288], dlen[32], clen[20];
    uint16_t rle[320];
    uint16_t entry[UQ_DEF_NSUB];
    uint32_t nrle, hlit, hdist, hclen, hdr_bits, member_bytes, stored, body_bits;
};

// level 2: the level-1 state, the pre-round newest position (+ 1) of every position of the round, and the last match of a round
// (((position in the round + 1) << 16) | (distance - 1); 0 = none): one word read, the other written, swapped every round
struct UqDeflateLds2 : UqDeflateLds {
    uint16_t prev[UQ_DEF_ROUND];
    uint32_t rep[2];
};
struct UqDeflateSizeLds2 : UqDeflateSizeLds {
    uint16_t prev[UQ_DEF_ROUND];
    uint32_t rep[2];
};

UQ_DEF_HD uint32_t uq_def_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }

// the length of a len[] code, and the code of a length
UQ_DEF_HD uint32_t uq_def_mlen(uint32_t v) { return v == 255 ? 258u : v + 2; }
UQ_DEF_HD uint32_t uq_def_lcode(uint32_t L) { return L == 258 ? 255u : (L > 256 ? 254u : L - 2); }

// literal/length symbol of a match length (3..258), with its extra bits (value, count)
UQ_DEF_HD uint32_t uq_def_lsym(uint32_t L, uint32_t& ev, uint32_t& en) {
    if (L == 258) { ev = 0; en = 0; return 285; }
    if (L <= 10) { ev = 0; en = 0; return 254 + L; }
    const uint32_t l = L - 3, ex = uq_def_log2(l) - 2, base = l >> ex;
    ev = l - (base << ex); en = ex;
    return 257 + 4 * (ex + 1) + (base - 4);
}

// distance symbol of a distance (1..32768), with its extra bits
UQ_DEF_HD uint32_t uq_def_dsym(uint32_t D, uint32_t& ev, uint32_t& en) {
    const uint32_t d = D - 1;
    if (d < 4) { ev = 0; en = 0; return d; }
    const uint32_t l = uq_def_log2(d), ex = l - 1, sym = 2 * l + ((d >> ex) & 1);
    ev = d - ((2u + (sym & 1)) << ex); en = ex;
    return sym;
}

// the extra bits of a literal/length symbol (0..285) and of a distance symbol (0..29)
UQ_DEF_HD uint32_t uq_def_lextra(uint32_t sym) { return sym < 265 || sym == 285 ? 0u : (sym - 261) >> 2; }
UQ_DEF_HD uint32_t uq_def_dextra(uint32_t sym) { return sym < 4 ? 0u : (sym >> 1) - 1; }


UQ_DEF_HD uint32_t uq_def_hash(const uint8_t* p) {
    const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    return (v * 2654435761u) >> (32 - UQ_DEF_HASH_BITS);
}

// the bytes (at most lim) that in[c...] and in[p...] share, c < p
UQ_DEF_HD uint32_t uq_def_common(const uint8_t* in, uint32_t c, uint32_t p, uint32_t lim) {
    uint32_t L = 0;
    while (L < lim && in[c + L] == in[p + L]) ++L;
    return L;
}

// the token at p as the parse takes it: 0 = a literal, else the len[] code of its match.  Level 2 is lazy: a match shorter than
// UQ_DEF_LAZY_MAX gives way to a longer one at p + 1 (len[] codes order as lengths do).
template <int kLevel>
UQ_DEF_HD uint32_t uq_def_tok(const uint8_t* len, uint32_t p, uint32_t n) {
    const uint32_t v = len[p];
    if constexpr (kLevel >= 2) {
        if (v && v < UQ_DEF_LAZY_MAX - 2 && p + 1 < n && len[p + 1] > v) return 0;
    }
    return v;
}

// A range of the member's bits [b0, b1) written word by word through Env: whole words stored, the partial words at either end OR-ed.
template <class Env>
struct UqDefBits {
    Env& env;
    uint64_t acc;
    uint32_t nacc, w;
    bool partial;
    UQ_DEF_HD UqDefBits(Env& e, uint32_t b0) : env(e), acc(0), nacc(b0 & 31), w(b0 >> 5), partial((b0 & 31) != 0) {}
    UQ_DEF_HD void put(uint32_t v, uint32_t n) {        // n <= 32, v < 2^n
        acc |= (uint64_t)v << nacc;
        nacc += n;
        if (nacc >= 32) {
            if (partial) env.word_or(w, (uint32_t)acc); else env.word_store(w, (uint32_t)acc);
            partial = false;
            acc >>= 32; nacc -= 32; ++w;
        }
    }
    UQ_DEF_HD void finish() { if (nacc) env.word_or(w, (uint32_t)acc); }                // a partial last word
};

// Code lengths (limit bits at most) of the n symbols with weights freq[] into lens[]; a complete code of >= 2 symbols whatever the weights.
// Lengths come from a Huffman tree over the symbols sorted by (weight, symbol) (ties: a leaf before an internal node); when its depth passes
// the limit, weights below t are raised to t and the tree is rebuilt, t = 2, 4, 8, ...  All threads call it; thread 0 builds the trees.
template <class Env>
UQ_DEF_HD void uq_def_huffman(Env& env, const uint32_t* freq, uint32_t n, uint32_t limit, uint8_t* lens, UqDefHuffScratch* h, uint32_t tid,
                              uint32_t nth) {
    for (uint32_t s = tid; s < n; s += nth) lens[s] = 0;
    if (tid == 0) h->done = 0;
    env.sync();
    for (uint32_t t = 1, it = 0; it < 32; t <<= 1, ++it) {
        // rank of every weighted symbol (weights clamped to >= t)
        for (uint32_t s = tid; s < n; s += nth) {
            const uint32_t f = freq[s];
            if (!f) continue;
            const uint32_t w = f > t ? f : t;
            uint32_t r = 0;
            for (uint32_t q = 0; q < n; ++q) {
                const uint32_t fq = freq[q];
                const uint32_t wq = fq > t ? fq : t;
                r += (uint32_t)(fq != 0 && (wq < w || (wq == w && q < s)));
            }
            h->sorted[r] = (uint16_t)s;
        }
        env.sync();
        if (tid == 0) {
            uint32_t m = 0;
            for (uint32_t s = 0; s < n; ++s) m += (uint32_t)(freq[s] != 0);
            if (m < 2) {
                const uint32_t a = m ? h->sorted[0] : 0, b = a == 0 ? 1 : 0;
                lens[a] = 1; lens[b] = 1;
                h->done = 1;
            } else {
                for (uint32_t i = 0; i < m; ++i) { const uint32_t f = freq[h->sorted[i]]; h->weight[i] = f > t ? f : t; }
                uint32_t li = 0, ni = m;                                        // next leaf, next internal node to consume
                for (uint32_t k = m; k < 2 * m - 1; ++k) {
                    uint32_t pick[2];
                    for (int j = 0; j < 2; ++j) {
                        if (li < m && (ni >= k || h->weight[li] <= h->weight[ni])) pick[j] = li++;
                        else pick[j] = ni++;
                    }
                    h->weight[k] = h->weight[pick[0]] + h->weight[pick[1]];
                    h->parent[pick[0]] = (uint16_t)k; h->parent[pick[1]] = (uint16_t)k;
                }
                h->depth[2 * m - 2] = 0;
                uint32_t maxd = 0;
                for (uint32_t k = 2 * m - 2; k-- > 0;) {
                    const uint32_t d = h->depth[h->parent[k]] + 1u;
                    h->depth[k] = (uint8_t)(d > 255 ? 255 : d);
                    if (k < m && d > maxd) maxd = d;
                }
                if (maxd <= limit) {
                    for (uint32_t i = 0; i < m; ++i) lens[h->sorted[i]] = h->depth[i];
                    h->done = 1;
                }
            }
        }
        env.sync();
        const uint32_t fin = h->done;
        env.sync();                                                     // every thread has read `done` before the next call resets it
        if (fin) break;
    }
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for LSB-first output; thread 0
UQ_DEF_HD void uq_def_codes(const uint8_t* lens, uint32_t n, uint16_t* codes) {
    uint32_t count[16] = {0}, next[16];
    for (uint32_t s = 0; s < n; ++s) count[lens[s]]++;
    count[0] = 0;
    uint32_t code = 0;
    for (int l = 1; l < 16; ++l) { code = (code + count[l - 1]) << 1; next[l] = code; }
    for (uint32_t s = 0; s < n; ++s)
        codes[s] = lens[s] ? (uint16_t)uq_inf_rev(next[lens[s]]++, lens[s]) : 0;
}

// Phases 1 to 5 on s->in[0, n) (n <= UQ_DEF_MAX_IN): the member's size in s->member_bytes, stored or dynamic in s->stored, visible to all
// threads on return.  kEmit (Lds = UqDeflateLds) also leaves what phase 6 writes the member from: the CRC, the codes, every sub-segment's
// first bit.  Without it (Lds = UqDeflateSizeLds) the same matches, parse, histograms and code lengths are computed and nothing else: the
// distance workspace holds distance symbols (one byte per position will do: Env::dist_put / dist_get take and give the symbol), and the
// bits of the tokens are counted from the histograms (sum of frequency x (code length + extra bits)) instead of by a second walk.
template <bool kEmit, int kLevel = 1, class Env, class Lds>
UQ_DEF_HD void uq_def_plan(Env& env, Lds* s, uint32_t n, uint32_t tid, uint32_t nth) {
    if constexpr (kEmit)
        for (uint32_t e = tid; e < 256; e += nth) s->crctab[e] = uq_crc_table_entry(e);
    for (uint32_t e = tid; e < (1u << UQ_DEF_HASH_BITS); e += nth) s->u.head[e] = 0;
    for (uint32_t e = tid; e < 288; e += nth) s->lfreq[e] = 0;
    for (uint32_t e = tid; e < 32; e += nth) s->dfreq[e] = 0;
    for (uint32_t e = tid; e < 20; e += nth) s->cfreq[e] = 0;
    for (uint32_t e = tid; e < 16; e += nth) s->in[n + e] = 0;
    if constexpr (kEmit) { if (tid == 0) s->crc0 = 0; } else { if (tid == 0) s->body_bits = 0; }
    if constexpr (kLevel >= 2) { if (tid == 0) { s->rep[0] = 0; s->rep[1] = 0; } }
    env.sync();

    // ---- 1. CRC-32
    if constexpr (kEmit) {
        const uint32_t S = (n + nth - 1) / nth;
        const uint32_t lo = tid * S < n ? tid * S : n, hi = lo + S < n ? lo + S : n;
        uint32_t c = uq_crc0_bytes(s->crctab, 0, s->in + lo, hi - lo);
        if (hi > lo) env.lds_xor(&s->crc0, uq_crc_multmodp(uq_crc_shift_op(env.x2n, n - hi), c));
    }

    // ---- 2. matches, round by round
    const uint32_t nrounds = (n + UQ_DEF_ROUND - 1) / UQ_DEF_ROUND;
    for (uint32_t r = 0; r < nrounds; ++r) {
        const uint32_t r0 = r * UQ_DEF_ROUND, r1 = r0 + UQ_DEF_ROUND < n ? r0 + UQ_DEF_ROUND : n;
        if constexpr (kLevel == 1) {
            for (uint32_t p = r0 + tid; p < r1; p += nth) {
                uint32_t v = 0;
                if (p + 4 <= n) {
                    const uint32_t c1 = s->u.head[uq_def_hash(s->in + p)];
                    if (c1 && p - (c1 - 1) <= 32768u) {
                        const uint32_t c = c1 - 1, lim = n - p < 258 ? n - p : 258;
                        uint32_t L = 0;
                        while (L < lim && s->in[c + L] == s->in[p + L]) ++L;
                        if (L >= 3 && !(L == 3 && p - c > 4096)) {
                            v = uq_def_lcode(L);
                            if constexpr (kEmit) env.dist_put(p, p - c);
                            else { uint32_t dv, dn; env.dist_put(p, uq_def_dsym(p - c, dv, dn)); }
                        }
                    }
                }
                s->len[p] = (uint8_t)v;
            }
            env.sync();
            for (uint32_t p = r0 + tid; p < r1; p += nth)
                if (p + 4 <= n) env.lds_max(&s->u.head[uq_def_hash(s->in + p)], p + 1);
            env.sync();
        } else {
            const uint32_t repw = s->rep[r & 1];
            for (uint32_t p = r0 + tid; p < r1; p += nth) {
                uint32_t v = 0;
                if (p + 3 <= n) {
                    // candidate distances, 0 = none: 1, 2, the head word's two positions, the last match of the round before
                    uint32_t cd[5] = {p >= 1 ? 1u : 0u, p >= 2 ? 2u : 0u, 0, 0, repw ? (repw & 0xFFFFu) + 1 : 0u};
                    if (p + 4 <= n) {
                        const uint32_t h = s->u.head[uq_def_hash(s->in + p)];
                        s->prev[p - r0] = (uint16_t)(h >> 16);
                        if (h >> 16) cd[2] = p - ((h >> 16) - 1);
                        if (h & 0xFFFFu) cd[3] = p - ((h & 0xFFFFu) - 1);
                    }
                    const uint32_t lim = n - p < 258 ? n - p : 258;
                    uint32_t bl = 0, bd = 0;
                    for (uint32_t k = 0; k < 5; ++k) {
                        const uint32_t d = cd[k];
                        if (!d || d > p || d > 32768u) continue;
                        const uint32_t L = uq_def_common(s->in, p - d, p, lim);
                        if (L > bl || (L == bl && d < bd)) { bl = L; bd = d; }
                    }
                    if (bl >= 3 && !(bl == 3 && bd > 4096)) {
                        v = uq_def_lcode(bl);
                        if constexpr (kEmit) env.dist_put(p, bd);
                        else { uint32_t dv, dn; env.dist_put(p, uq_def_dsym(bd, dv, dn)); }
                        env.lds_max(&s->rep[(r + 1) & 1], ((p - r0 + 1) << 16) | (bd - 1));
                    }
                }
                s->len[p] = (uint8_t)v;
            }
            env.sync();
            for (uint32_t p = r0 + tid; p < r1; p += nth)
                if (p + 4 <= n) env.lds_max(&s->u.head[uq_def_hash(s->in + p)], ((p + 1) << 16) | s->prev[p - r0]);
            if (tid == 0) s->rep[r & 1] = 0;
            env.sync();
        }
    }

    // ---- 3. parse (greedy; level 2: lazy, see uq_def_tok): the first token start of every sub-segment
    const uint32_t nsub = (n + UQ_DEF_SUB - 1) / UQ_DEF_SUB;
    uint32_t cur = 0;                                                   // thread 0: the chain's next token start
    for (uint32_t w0 = 0; w0 < n; w0 += UQ_DEF_WIN) {
        const uint32_t w1 = w0 + UQ_DEF_WIN < n ? w0 + UQ_DEF_WIN : n;
        for (uint32_t p = w0 + tid; p < w1; p += nth) {
            const uint32_t v = uq_def_tok<kLevel>(s->len, p, n);
            s->u.jmp[p - w0] = (uint16_t)(p + (v ? uq_def_mlen(v) : 1) - w0);
        }
        env.sync();
        for (uint32_t k = 1; k < UQ_DEF_SUB; k <<= 1) {                 // log2(UQ_DEF_SUB) rounds: chains inside a sub-segment are that short
            for (uint32_t p = w0 + tid; p < w1; p += nth) {
                const uint32_t e = (p / UQ_DEF_SUB + 1) * UQ_DEF_SUB, end = e < n ? e : n;
                const uint32_t j = s->u.jmp[p - w0] + w0;
                if (j < end) s->u.jmp[p - w0] = s->u.jmp[j - w0];
            }
            env.sync();
        }
        if (tid == 0) {
            for (uint32_t k = w0 / UQ_DEF_SUB; k * UQ_DEF_SUB < w1; ++k) {
                const uint32_t e = (k + 1) * UQ_DEF_SUB, end = e < n ? e : n;
                if (cur < end) { s->entry[k] = (uint16_t)cur; cur = s->u.jmp[cur - w0] + w0; }
                else s->entry[k] = UQ_DEF_NONE;
            }
        }
        env.sync();
    }

    // ---- 4. histograms, codes
    for (uint32_t k = tid; k < nsub; k += nth) {
        const uint32_t end = (k + 1) * UQ_DEF_SUB < n ? (k + 1) * UQ_DEF_SUB : n;
        for (uint32_t p = s->entry[k]; p < end;) {
            const uint32_t v = uq_def_tok<kLevel>(s->len, p, n);
            if (!v) { env.lds_add(&s->lfreq[s->in[p]], 1); ++p; continue; }
            uint32_t ev, en;
            const uint32_t L = uq_def_mlen(v);
            env.lds_add(&s->lfreq[uq_def_lsym(L, ev, en)], 1);
            if constexpr (kEmit) env.lds_add(&s->dfreq[uq_def_dsym(env.dist_get(p), ev, en)], 1);
            else env.lds_add(&s->dfreq[env.dist_get(p)], 1);
            p += L;
        }
    }
    if (tid == 0) s->lfreq[256] = 1;
    env.sync();
    uq_def_huffman(env, s->lfreq, 286, 15, s->llen, &s->u.h, tid, nth);
    uq_def_huffman(env, s->dfreq, 30, 15, s->dlen, &s->u.h, tid, nth);
    if (tid == 0) {
        if constexpr (kEmit) {
            uq_def_codes(s->llen, 286, s->lcode);
            uq_def_codes(s->dlen, 30, s->dcode);
        }
        uint32_t hlit = 286, hdist = 30;
        while (hlit > 257 && !s->llen[hlit - 1]) --hlit;
        while (hdist > 1 && !s->dlen[hdist - 1]) --hdist;
        // run-length code of the hlit + hdist lengths (one sequence: runs may cross from one code into the other)
        uint32_t nr = 0, i = 0, prev = 16;
        const uint32_t tot = hlit + hdist;
        while (i < tot) {
            const uint32_t l = i < hlit ? s->llen[i] : s->dlen[i - hlit];
            uint32_t run = 1;
            while (run < 138 && i + run < tot && (i + run < hlit ? s->llen[i + run] : s->dlen[i + run - hlit]) == l) ++run;
            if (l == 0 && run >= 3) {                                   // 17: 3..10 zeros, 18: 11..138
                s->rle[nr] = run <= 10 ? 17 : 18;
                if constexpr (kEmit) s->rlex[nr] = (uint8_t)(run <= 10 ? run - 3 : run - 11);
                ++nr; i += run; prev = 0;
            } else if (l == prev && run >= 3) {                          // 16: the previous length 3..6 times more
                const uint32_t r = run > 6 ? 6 : run;
                s->rle[nr] = 16;
                if constexpr (kEmit) s->rlex[nr] = (uint8_t)(r - 3);
                ++nr; i += r;
            } else {
                s->rle[nr] = (uint16_t)l;
                if constexpr (kEmit) s->rlex[nr] = 0;
                ++nr; ++i; prev = l;
            }
        }
        for (uint32_t k = 0; k < nr; ++k) s->cfreq[s->rle[k]]++;
        s->nrle = nr; s->hlit = hlit; s->hdist = hdist;
    }
    env.sync();
    uq_def_huffman(env, s->cfreq, 19, 7, s->clen, &s->u.h, tid, nth);
    if (tid == 0) {
        if constexpr (kEmit) uq_def_codes(s->clen, 19, s->ccode);
        uint32_t hclen = 19;
        while (hclen > 4 && !s->clen[uq_inf_order(hclen - 1)]) --hclen;
        uint32_t b = 3 + 5 + 5 + 4 + 3 * hclen;
        for (uint32_t k = 0; k < s->nrle; ++k) {
            const uint32_t sym = s->rle[k];
            b += s->clen[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
        }
        s->hclen = hclen; s->hdr_bits = b;
    }
    env.sync();

    // ---- 5. bits of every sub-segment, the member's size, stored or not
    if constexpr (kEmit) {
        for (uint32_t k = tid; k < nsub; k += nth) {
            const uint32_t end = (k + 1) * UQ_DEF_SUB < n ? (k + 1) * UQ_DEF_SUB : n;
            uint32_t b = 0;
            for (uint32_t p = s->entry[k]; p < end;) {
                const uint32_t v = uq_def_tok<kLevel>(s->len, p, n);
                if (!v) { b += s->llen[s->in[p]]; ++p; continue; }
                uint32_t ev, en, dv, dn;
                const uint32_t L = uq_def_mlen(v);
                const uint32_t ls = uq_def_lsym(L, ev, en), ds = uq_def_dsym(env.dist_get(p), dv, dn);
                b += s->llen[ls] + en + s->dlen[ds] + dn;
                p += L;
            }
            s->bits[k] = b;
        }
        env.sync();
        if (tid == 0) {
            uint32_t off = 144 + s->hdr_bits;
            for (uint32_t k = 0; k < nsub; ++k) { const uint32_t b = s->bits[k]; s->bits[k] = off; off += b; }
            s->bits[nsub] = off;                                            // end-of-block code, padding, trailer
            const uint32_t dyn = 18 + (off + s->llen[256] - 144 + 7) / 8 + 8, stored = 18 + 5 + n + 8;
            s->stored = stored <= dyn;
            s->member_bytes = s->stored ? stored : dyn;
        }
        env.sync();
    } else {
        // a token's bits are its symbols' code lengths and extra bits; lfreq[256] = 1 stands for the end-of-block code
        uint32_t b = 0;
        for (uint32_t e = tid; e < 286; e += nth) b += s->lfreq[e] * (s->llen[e] + uq_def_lextra(e));
        for (uint32_t e = tid; e < 30; e += nth) b += s->dfreq[e] * (s->dlen[e] + uq_def_dextra(e));
        if (b) env.lds_add(&s->body_bits, b);
        env.sync();
        if (tid == 0) {
            const uint32_t dyn = 18 + (s->hdr_bits + s->body_bits + 7) / 8 + 8, stored = 18 + 5 + n + 8;
            s->stored = stored <= dyn;
            s->member_bytes = s->stored ? stored : dyn;
        }
        env.sync();
    }
}

// The size of the BGZF member that uq_deflate_block writes for s->in[0, n), and nothing written.  Env: sync(), lds_max / lds_add, and
// dist_put(p, sym) / dist_get(p) (one distance symbol, 0..29, per position: n entries).  The block must already be in s->in.
// uq_deflate_block_size_l<2> (Lds = UqDeflateSizeLds2): the size uq_deflate_block_l<2> writes.
template <int kLevel, class Env, class Lds>
UQ_DEF_HD int uq_deflate_block_size_l(Env& env, Lds* s, uint32_t n, uint32_t tid, uint32_t nth, uint32_t* member_bytes) {
    if (n > UQ_DEF_MAX_IN) return UQ_DEF_TOO_LARGE;
    uq_def_plan<false, kLevel>(env, s, n, tid, nth);
    *member_bytes = s->member_bytes;
    return UQ_DEF_OK;
}
template <class Env>
UQ_DEF_HD int uq_deflate_block_size(Env& env, UqDeflateSizeLds* s, uint32_t n, uint32_t tid, uint32_t nth, uint32_t* member_bytes) {
    return uq_deflate_block_size_l<1>(env, s, n, tid, nth, member_bytes);
}

// Compresses s->in[0, n) into one BGZF member: *member_bytes = its size.  Env: sync(), lds_max / lds_add / lds_xor (atomics on LDS words),
// dist_put(p, d) / dist_get(p) (the distance workspace, n entries), word_store(w, v) / word_or(w, v) (32-bit word w of the member; the member's
// words are zero before the call), and x2n (the CRC shift table).  The block must already be in s->in.
// uq_deflate_block_l<2> (Lds = UqDeflateLds2): level 2, the same Env.
template <int kLevel, class Env, class Lds>
UQ_DEF_HD int uq_deflate_block_l(Env& env, Lds* s, uint32_t n, uint32_t cap, uint32_t tid, uint32_t nth, uint32_t* member_bytes) {
    if (n > UQ_DEF_MAX_IN) return UQ_DEF_TOO_LARGE;
    uq_def_plan<true, kLevel>(env, s, n, tid, nth);
    const uint32_t nsub = (n + UQ_DEF_SUB - 1) / UQ_DEF_SUB;
    const uint32_t mb = s->member_bytes;
    *member_bytes = mb;
    if (mb > cap) return UQ_DEF_NO_SPACE;
    const uint32_t crc = uq_crc_finish(env.x2n, s->crc0, n);

    // the gzip header: ID1 ID2 CM FLG MTIME(4) XFL OS XLEN(2) 'B' 'C' SLEN(2) BSIZE(2)
    const uint32_t h0 = 0x04088b1fu, h1 = 0, h2 = 0x0006ff00u, h3 = 0x00024342u, bsize = mb - 1;
    if (s->stored) {
        // ---- stored block: 01 LEN NLEN, the bytes, the trailer
        const uint32_t nw = (mb + 3) / 4;
        for (uint32_t w = tid; w < nw; w += nth) {
            uint32_t v = 0;
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t j = 4 * w + k;
                uint32_t b;
                if (j < 16) { const uint32_t hw = j < 4 ? h0 : j < 8 ? h1 : j < 12 ? h2 : h3; b = (hw >> (8 * (j & 3))) & 0xFF; }
                else if (j < 18) b = (bsize >> (8 * (j - 16))) & 0xFF;
                else if (j == 18) b = 1;
                else if (j < 21) b = (n >> (8 * (j - 19))) & 0xFF;
                else if (j < 23) b = ((n ^ 0xFFFF) >> (8 * (j - 21))) & 0xFF;
                else if (j < 23 + n) b = s->in[j - 23];
                else if (j < 27 + n) b = (crc >> (8 * (j - 23 - n))) & 0xFF;
                else if (j < 31 + n) b = (n >> (8 * (j - 27 - n))) & 0xFF;
                else b = 0;
                v |= b << (8 * k);
            }
            env.word_store(w, v);
        }
        return UQ_DEF_OK;
    }

    // ---- 6. the dynamic block: header staged by thread 0, then every range by one thread
    if (tid == 0) {
        for (uint32_t w = 0; w < UQ_DEF_HDR_WORDS; ++w) s->hdr[w] = 0;
        s->hdr[0] = h0; s->hdr[1] = h1; s->hdr[2] = h2; s->hdr[3] = h3; s->hdr[4] = bsize & 0xFFFF;
        uint32_t bp = 144;
        auto put = [&](uint32_t v, uint32_t nb) {
            for (uint32_t k = 0; k < nb; ++k, ++bp) s->hdr[bp >> 5] |= ((v >> k) & 1u) << (bp & 31);
        };
        put(1, 1); put(2, 2);                                           // BFINAL, BTYPE = 10
        put(s->hlit - 257, 5); put(s->hdist - 1, 5); put(s->hclen - 4, 4);
        for (uint32_t k = 0; k < s->hclen; ++k) put(s->clen[uq_inf_order(k)], 3);
        for (uint32_t k = 0; k < s->nrle; ++k) {
            const uint32_t sym = s->rle[k];
            put(s->ccode[sym], s->clen[sym]);
            if (sym == 16) put(s->rlex[k], 2); else if (sym == 17) put(s->rlex[k], 3); else if (sym == 18) put(s->rlex[k], 7);
        }
    }
    env.sync();
    // ranges: 0 = header [0, bits[0]), 1 + k = sub-segment k, nsub + 1 = end-of-block code + padding + trailer
    for (uint32_t r = tid; r < nsub + 2; r += nth) {
        if (r == 0) {
            const uint32_t b1 = s->bits[0];
            UqDefBits<Env> bw(env, 0);
            for (uint32_t w = 0; 32 * w < b1; ++w) {
                const uint32_t nb = b1 - 32 * w < 32 ? b1 - 32 * w : 32;
                bw.put(nb == 32 ? s->hdr[w] : s->hdr[w] & ((1u << nb) - 1), nb);
            }
            bw.finish();
        } else if (r == nsub + 1) {
            UqDefBits<Env> bw(env, s->bits[nsub]);
            bw.put(s->lcode[256], s->llen[256]);
            const uint32_t e = s->bits[nsub] + s->llen[256];
            if (e & 7) bw.put(0, 8 - (e & 7));
            bw.put(crc, 32);
            bw.put(n, 32);
            bw.finish();
        } else {
            const uint32_t k = r - 1, end = (k + 1) * UQ_DEF_SUB < n ? (k + 1) * UQ_DEF_SUB : n;
            UqDefBits<Env> bw(env, s->bits[k]);
            for (uint32_t p = s->entry[k]; p < end;) {
                const uint32_t v = uq_def_tok<kLevel>(s->len, p, n);
                if (!v) { const uint32_t c = s->in[p]; bw.put(s->lcode[c], s->llen[c]); ++p; continue; }
                uint32_t ev, en, dv, dn;
                const uint32_t L = uq_def_mlen(v);
                const uint32_t ls = uq_def_lsym(L, ev, en), ds = uq_def_dsym(env.dist_get(p), dv, dn);
                bw.put(s->lcode[ls], s->llen[ls]);
                if (en) bw.put(ev, en);
                bw.put(s->dcode[ds], s->dlen[ds]);
                if (dn) bw.put(dv, dn);
                p += L;
            }
            bw.finish();
        }
    }
    return UQ_DEF_OK;
}

template <class Env>
UQ_DEF_HD int uq_deflate_block(Env& env, UqDeflateLds* s, uint32_t n, uint32_t cap, uint32_t tid, uint32_t nth, uint32_t* member_bytes) {
    return uq_deflate_block_l<1>(env, s, n, cap, tid, nth, member_bytes);
}
