"""A token-level deflate writer for the tests of the three inflate paths, and the case lists made with it.

Every valid stream in the rest of the suite comes from zlib's compressor or from the project's own one; zlib's compressor never writes a
distance above 32 506 (w_size - 262), almost never a code longer than 13 bits on FASTQ, never length 258 as symbol 284 + 31, never a repeat
of a zero length with symbol 16, and so on.  This writer writes any valid raw deflate stream (RFC 1951) from a description -- blocks of
literal and (length, distance) tokens with explicit or policy-made code lengths -- and replays the tokens into the expected output.  zlib's
*inflate* is the reference: `deflate()` asserts that zlib.decompressobj(-15) inflates the stream to exactly the replayed bytes, with eof
set and nothing unused; the replay only guards the writer itself.  Nothing here is skipped: a case zlib refuses is an assertion error.

Where each edge of the issue lives (crafted_members = M, crafted_streams = S, crafted_invalid = I):

  distances above 32 506, extra bits of distance symbol 29      M dist_sym29_last_extra_bits, M random/*
  reference to output position 0 from 32 768                    M dist_32768_to_position_0
  chunk decoder: the oldest ring entry (marker w = 0)           S marker_oldest_ring_entry
  a match whose source wraps the ring                           S source_wraps_the_ring, S all_matches_at_32768
  14 and 15-bit literal/length codes, 9 to 15-bit distance      M lit_codes_to_15_bits, M lit_codes_15_bits_frequent, M dist_codes_to_15_bits,
  codes (the canonical slow path)                               M both_codes_deep, M random/*
  length 258 as symbol 284 + extra 31                           M len_258_as_284_31
  a distance code of one 1-bit code                             M dist_single_one_bit_code
  no distance code at all                                       M dist_none_literal_only
  a literal/length code that is only end-of-block               M lit_only_end_of_block
  HLIT / HDIST / HCLEN minima                                   M hlit_257_hdist_1_hclen_5 (HCLEN 4 leaves only zero lengths, so it has no
                                                                end-of-block code: I hclen_4_only_zero_lengths)
  a code-length code that is not complete: one code of one    I precode_only_16_then_16, I precode_only_8_then_ones, I precode_only_0_then_zeros,
  bit, or none (both decoders: status 4 before any repeat,    I precode_hclen_4_all_zero
  symbol or end-of-block check)
  HLIT / HDIST / HCLEN maxima                                   M hlit_286_hdist_30_hclen_19
  16 straight after 17 / 18                                     M rle_16_after_17, M rle_16_after_18
  18 with 138                                                   M rle_18_with_138
  a run that ends exactly at the HLIT boundary (and one across) M rle_run_ends_at_hlit, M rle_run_crosses_hlit
  empty blocks of every type, several in a row                  M empty_blocks_of_every_type, S empty_dynamic_blocks_x64
  the empty fixed block of Z_PARTIAL_FLUSH                      M zlib_partial_flush, S zlib_partial_flush
  stored header at each of the 8 bit alignments                 M stored_header_at_bit_0 ... _7
  stored LEN 0 as the final block, LEN 65 535                   M stored_len_0_final, M stored_len_65535
  a stored block last after Huffman blocks                      M stored_last_after_huffman
  65 536 bytes of output ending inside a 258-byte match         M out_65536_ends_in_match_258
  dist == pos exactly, dist 1 len 258                           M dist_equals_pos, M dist_1_len_258
  an overlapping match whose source is markers                  S overlapping_match_of_markers
  a marker kept alive by a chain of copies                      S marker_chain_250k
  the switch at exactly 32 768 symbols after the last marker    S switch_at_exactly_32768, S switch_one_symbol_late, S chunk_ends_at_exactly_32768
  long runs of fixed blocks across chunks                       S fixed_only_200k
  a unit whose canonical position equals a chunk's stop         S dynamic_unit_at_chunk_boundary, S stored_unit_at_chunk_boundary
  a member that ends on the last bit of a chunk                 S member_ends_at_chunk_16384, S member_ends_at_chunk_6000
"""
import bisect
import functools
import gzip
import heapq
import random
import struct
import zlib

MAX_MEMBER = 65536
WINDOW = 32768
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
GZIP_HEADER = b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03'
BGZF_HEADER = b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00'


class Bits:
    """LSB-first bit writer for hand-made deflate streams."""

    def __init__(self):
        self.n = 0                                              # bits written
        self._done, self._v, self._k = bytearray(), 0, 0       # whole bytes so far; the pending bits and their count

    def put(self, value, n):
        self._v |= (value & ((1 << n) - 1)) << self._k
        self._k += n
        self.n += n
        if self._k >= 64:
            whole = self._k // 8
            self._done += (self._v & ((1 << (8 * whole)) - 1)).to_bytes(whole, 'little')
            self._v >>= 8 * whole
            self._k -= 8 * whole
        return self

    def code(self, code, n):                                # Huffman codes go most significant bit first
        return self.put(int(format(code, '0%db' % n)[::-1], 2), n)

    def align(self):
        return self.put(0, -self.n % 8)

    def raw(self, data):
        assert self.n % 8 == 0
        self._done += self._v.to_bytes(self._k // 8, 'little') + data
        self._v, self._k = 0, 0
        self.n += 8 * len(data)
        return self

    def bytes(self):
        return bytes(self._done) + self._v.to_bytes((self._k + 7) // 8, 'little')


def fixed_lit(b, s):
    if s < 144: b.code(0x30 + s, 8)
    elif s < 256: b.code(0x190 + s - 144, 9)
    elif s < 280: b.code(s - 256, 7)
    else: b.code(0xC0 + s - 280, 8)


# ------------------------------------------------------------------ symbols and code lengths
def length_symbol(length, alt258=False):
    """(symbol, extra value, extra bits) of a match length; alt258: 258 as 284 + 31 rather than 285"""
    assert 3 <= length <= 258
    if length == 258 and alt258:
        return 284, 31, 5
    i = bisect.bisect_right(LBASE, length) - 1
    return 257 + i, length - LBASE[i], LEXT[i]


def distance_symbol(dist):
    assert 1 <= dist <= 32768
    i = bisect.bisect_right(DBASE, dist) - 1
    return i, dist - DBASE[i], DEXT[i]


def canonical_codes(lens):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths (RFC 1951 3.2.2)"""
    count = [0] * 17
    for l in lens: count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def kraft(lens):
    """sum of 2^-l in units of 2^-15: 32 768 = complete"""
    return sum(1 << (15 - l) for l in lens if l)


def huffman_lengths(freq, limit):
    """Optimal code lengths of the symbols of `freq` (symbol -> count > 0), flattened until no length exceeds `limit`"""
    syms = sorted(freq)
    if len(syms) == 1:
        return {syms[0]: 1}
    f = dict(freq)
    while True:
        # nodes 0 .. n - 1 are the leaves; ties go to the subtree with the smaller least symbol
        heap = [(f[s], s, i) for i, s in enumerate(syms)]
        heapq.heapify(heap)
        parent = [None] * len(syms)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            parent[a[2]] = parent[b[2]] = len(parent)
            parent.append(None)
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), len(parent) - 1))
        level = [0] * len(parent)
        for i in range(len(parent) - 2, -1, -1): level[i] = level[parent[i]] + 1
        if max(level[:len(syms)]) <= limit:
            return dict(zip(syms, level))
        f = {s: (c + 1) // 2 for s, c in f.items()}


def comb_depths(k, limit):
    """k leaf depths of a complete tree that is as deep as it can be: the comb 1, 2, ..., limit, limit, its shallowest leaves split for more"""
    if k == 1:
        return [1]
    d = list(range(1, min(k, limit + 1))) + [min(k - 1, limit)]
    while len(d) < k:
        d.sort()
        d[0:1] = [d[0] + 1, d[0] + 1]
    return sorted(d)


def policy_lengths(policy, freq, nsyms, limit=15):
    """The code lengths (a list of nsyms) that `policy` gives the used symbols of `freq`.
    'huffman', 'deep' (comb, frequent symbols short), 'deep_rev' (comb, frequent symbols long), ('random', seed, max_len), 'single', 'none',
    or the explicit list itself."""
    if isinstance(policy, (list, tuple)) and not (policy and policy[0] == 'random'):
        lens = list(policy) + [0] * (nsyms - len(policy))
        assert len(lens) == nsyms and all(lens[s] for s in freq), 'a used symbol has no code'
        return lens
    lens = [0] * nsyms
    used = sorted(freq, key=lambda s: (-freq[s], s))
    if policy == 'none':
        assert not used
        return lens
    if policy == 'single':
        assert len(used) == 1
        lens[used[0]] = 1
        return lens
    if not used:
        return lens
    if policy == 'huffman':
        for s, l in huffman_lengths(freq, limit).items(): lens[s] = l
        return lens
    if policy in ('deep', 'deep_rev'):
        spare = [s for s in range(nsyms) if s not in freq]
        if len(used) == 1 and not spare:
            lens[used[0]] = 1
            return lens
        pads = min(max(0, limit + 1 - len(used)), len(spare))
        depths = comb_depths(len(used) + pads, limit)
        # the unused symbols take the short codes, so that the stream's own symbols carry the long ones
        for s, l in zip(spare[len(spare) - pads:], depths[:pads]): lens[s] = l
        mine = depths[pads:]
        for s, l in zip(used, mine if policy == 'deep' else mine[::-1]): lens[s] = l
        return lens
    assert policy[0] == 'random'
    _, seed, max_len = policy
    rnd = random.Random(seed)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    assert len(used) <= 1 << max_len
    leaves = [0]
    while len(leaves) < len(used):
        open_ = [i for i, d in enumerate(leaves) if d < max_len]
        i = rnd.choice(open_)
        leaves[i:i + 1] = [leaves[i] + 1, leaves[i] + 1]
    rnd.shuffle(leaves)
    for s, l in zip(sorted(used), leaves): lens[s] = l
    return lens


def rle_ops(seq, mode='greedy', seed=0):
    """The code-length sequence as (symbol, extra value) ops of the code-length alphabet.  mode: 'none' (every length by itself), 'greedy'
    (the longest 16 / 17 / 18 runs), 'random', 'zero16_17' / 'zero16_18' (zero runs as one 17 / 18 and then 16s: a repeated zero)."""
    rnd = random.Random(seed)
    ops, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        run = 1
        while i + run < n and seq[i + run] == v: run += 1
        prev_same = i > 0 and seq[i - 1] == v
        if mode == 'none':
            ops.append((v, 0)); i += 1
        elif mode == 'greedy':
            if v == 0 and run >= 11: k = min(run, 138); ops.append((18, k - 11)); i += k
            elif v == 0 and run >= 3: k = min(run, 10); ops.append((17, k - 3)); i += k
            elif prev_same and run >= 3: k = min(run, 6); ops.append((16, k - 3)); i += k
            else: ops.append((v, 0)); i += 1
        elif mode in ('zero16_17', 'zero16_18'):
            first = 3 if mode == 'zero16_17' else 11
            if v == 0 and prev_same and run >= 3: k = min(run, 6); ops.append((16, k - 3)); i += k
            elif v == 0 and run >= first + 3: ops.append((17, 0) if first == 3 else (18, 0)); i += first
            elif prev_same and run >= 3: k = min(run, 6); ops.append((16, k - 3)); i += k
            else: ops.append((v, 0)); i += 1
        else:
            assert mode == 'random'
            choices = [(v, 1)]
            if prev_same and run >= 3: choices.append((16, rnd.randint(3, min(run, 6))))
            if v == 0 and run >= 3: choices.append((17, rnd.randint(3, min(run, 10))))
            if v == 0 and run >= 11: choices += [(18, rnd.randint(11, min(run, 138))), (18, min(run, 138))]
            sym, k = rnd.choice(choices)
            ops.append((sym, 0 if sym < 16 else k - {16: 3, 17: 3, 18: 11}[sym])); i += k
    return ops


def replay_ops(ops):
    seq = []
    for sym, extra in ops:
        if sym < 16: seq.append(sym)
        elif sym == 16: seq += [seq[-1]] * (3 + extra)
        elif sym == 17: seq += [0] * (3 + extra)
        else: seq += [0] * (11 + extra)
    return seq


# ------------------------------------------------------------------ blocks and the writer
class Block:
    """One deflate block.  kind: 'stored' | 'fixed' | 'dynamic'; tokens: literals (ints) and (length, distance) pairs, or bytes;
    final: BFINAL (None: set on the last block of a stream); lit / dist: a code-length policy (policy_lengths) or the explicit lengths;
    hlit / hdist / hclen: 'trim', 'max' or the count itself; rle: a mode of rle_ops, or the explicit ops; alt258: length 258 as 284 + 31."""

    def __init__(self, kind, tokens=(), final=None, lit='huffman', dist='huffman', hlit='trim', hdist='trim', hclen='trim', rle='greedy',
                 rle_seed=0, alt258=False):
        self.kind, self.tokens, self.final = kind, list(tokens), final
        self.lit, self.dist, self.hlit, self.hdist, self.hclen, self.rle, self.rle_seed, self.alt258 = lit, dist, hlit, hdist, hclen, rle, rle_seed, alt258


class Writer:
    """Writes blocks one after another; .bits.n is the stream's length in bits so far, .out the replayed output, .log one dict a dynamic
    block (its lengths and header ops)."""

    def __init__(self):
        self.bits, self.out, self.log, self.ended = Bits(), bytearray(), [], False

    def _replay(self, tokens):
        out = self.out
        for t in tokens:
            if isinstance(t, int):
                out.append(t)
            else:
                l, d = t
                assert 3 <= l <= 258 and 1 <= d <= len(out) and d <= WINDOW, (l, d, len(out))
                if d >= l:
                    out += out[len(out) - d:len(out) - d + l]
                else:
                    out += (bytes(out[-d:]) * (l // d + 1))[:l]

    def add(self, blk, final=False):
        assert not self.ended
        b = self.bits
        final = bool(blk.final) if blk.final is not None else final
        self.ended = final
        b.put(1 if final else 0, 1)
        if blk.kind == 'stored':
            data = bytes(blk.tokens)
            assert len(data) <= 65535
            b.put(0, 2).align().put(len(data), 16).put(len(data) ^ 0xFFFF, 16).raw(data)
            self.out += data
            return self
        syms, lfreq, dfreq = [], {256: 1}, {}
        for t in blk.tokens:
            if isinstance(t, int):
                syms.append((t, None)); lfreq[t] = lfreq.get(t, 0) + 1
            else:
                ls, ds = length_symbol(t[0], blk.alt258), distance_symbol(t[1])
                syms.append((ls, ds)); lfreq[ls[0]] = lfreq.get(ls[0], 0) + 1; dfreq[ds[0]] = dfreq.get(ds[0], 0) + 1
        if blk.kind == 'fixed':
            b.put(1, 2)
            llens, dlens = FIXED_LIT, FIXED_DIST
        else:
            assert blk.kind == 'dynamic'
            b.put(2, 2)
            llens = policy_lengths(blk.lit, lfreq, 286)
            dlens = policy_lengths(blk.dist, dfreq, 30)
            self._header(blk, llens, dlens)
        lcode, dcode = canonical_codes(llens), canonical_codes(dlens)
        for ls, ds in syms:
            if ds is None:
                b.code(*lcode[ls])
            else:
                b.code(*lcode[ls[0]]).put(ls[1], ls[2]).code(*dcode[ds[0]]).put(ds[1], ds[2])
        b.code(*lcode[256])
        self._replay(blk.tokens)
        return self

    def _header(self, blk, llens, dlens):
        b = self.bits
        for lens, what in ((llens, 'literal/length'), (dlens, 'distance')):
            k, n = kraft(lens), sum(1 for l in lens if l)
            assert k == 32768 or (n == 1 and k == 16384) or (n == 0 and what == 'distance'), 'the %s code is not one deflate allows' % what
        top = lambda lens, least: max([least] + [s + 1 for s, l in enumerate(lens) if l])
        hlit = {'trim': top(llens, 257), 'max': 286}.get(blk.hlit, blk.hlit)
        hdist = {'trim': top(dlens, 1), 'max': 30}.get(blk.hdist, blk.hdist)
        assert hlit >= top(llens, 257) and hdist >= top(dlens, 1)
        seq = list(llens[:hlit]) + list(dlens[:hdist])
        ops = rle_ops(seq, blk.rle, blk.rle_seed) if isinstance(blk.rle, str) else list(blk.rle)
        assert replay_ops(ops) == seq, 'the header ops do not give the code lengths'
        cfreq = {}
        for sym, _ in ops: cfreq[sym] = cfreq.get(sym, 0) + 1
        if len(cfreq) == 1:                                  # the code-length code must be complete: a second symbol, unused
            cfreq[(min(cfreq) + 1) % 19] = 1
        clens = [0] * 19
        for s, l in huffman_lengths(cfreq, 7).items(): clens[s] = l
        hclen = 19 if blk.hclen in ('max', 19) else max([4] + [i + 1 for i, s in enumerate(ORDER) if clens[s]])
        if blk.hclen not in ('trim', 'max'): hclen = max(hclen, blk.hclen)
        b.put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
        for s in ORDER[:hclen]: b.put(clens[s], 3)
        ccode = canonical_codes(clens)
        for sym, extra in ops:
            b.code(*ccode[sym])
            if sym >= 16: b.put(extra, {16: 2, 17: 3, 18: 7}[sym])
        self.log.append(dict(llens=llens, dlens=dlens, hlit=hlit, hdist=hdist, hclen=hclen, ops=ops, clens=clens))

    def finish(self):
        """(raw deflate, expected output), checked against zlib's inflate"""
        assert self.ended, 'no final block'
        return checked(self.bits.bytes(), bytes(self.out))


def checked(raw, data):
    d = zlib.decompressobj(-15)
    got = d.decompress(raw) + d.flush()
    assert got == data and d.eof and not d.unused_data, 'zlib disagrees with the writer'
    return raw, data


def deflate(blocks):
    """(raw deflate stream, expected output) of a list of Blocks; the last one is final unless the blocks say otherwise"""
    w = Writer()
    for i, blk in enumerate(blocks): w.add(blk, final=i == len(blocks) - 1)
    return w.finish()


def gzip_wrap(raw, data):
    return GZIP_HEADER + raw + struct.pack('<II', zlib.crc32(data), len(data) & 0xFFFFFFFF)


def bgzf_wrap(raw, data):
    assert len(data) <= MAX_MEMBER and 18 + len(raw) + 8 <= 65536
    return BGZF_HEADER + struct.pack('<H', 18 + len(raw) + 8 - 1) + raw + struct.pack('<II', zlib.crc32(data), len(data))


def filler(gap):
    """Fixed blocks (no matches) of exactly `gap` bits, gap >= 80: 10 + 8 a + 9 b bits for a short and b long literals"""
    assert gap >= 80
    b = (gap - 10) % 8
    a = (gap - 10 - 9 * b) // 8
    return [Block('fixed', [65 + k % 20 for k in range(a)] + [200 + k for k in range(b)])]


# ------------------------------------------------------------------ tokens
def text_tokens(rnd, start, want, limit, alphabet=b'ACGTN@+\nI#', single_dsym=None, no_match=False):
    """Random tokens for `want` more bytes of output after `start` bytes (never past `limit`): lengths weighted to 3, 4, 257, 258, distances
    to 1, 2, pos, 32 506, 32 507, 32 767, 32 768 wherever pos allows.  single_dsym: every distance from that one distance symbol."""
    toks, pos, end = [], start, min(limit, start + want)
    while pos < end:
        room = end - pos
        if no_match or pos == 0 or room < 3 or rnd.random() < 0.35:
            toks.append(alphabet[rnd.randrange(len(alphabet))]); pos += 1
            continue
        r = rnd.random()
        length = rnd.choice([3, 4, 257, 258]) if r < 0.6 else rnd.randint(3, 258)
        length = min(length, room)
        if single_dsym is not None:
            lo, hi = DBASE[single_dsym], min(pos, DBASE[single_dsym] + (1 << DEXT[single_dsym]) - 1)
            if lo > pos:
                toks.append(alphabet[rnd.randrange(len(alphabet))]); pos += 1
                continue
            dist = rnd.choice([lo, hi, rnd.randint(lo, hi)])
        else:
            r = rnd.random()
            if r < 0.6:
                dist = rnd.choice([d for d in (1, 2, pos, 32506, 32507, 32767, 32768) if d <= min(pos, WINDOW)])
            else:
                dist = rnd.randint(1, min(pos, WINDOW))
        toks.append((length, dist)); pos += length
    return toks, pos


def random_policy(rnd, k_used):
    p = rnd.choice(['huffman', 'deep', 'deep_rev', 'random', 'random'])
    if p == 'random':
        need = max(1, (max(k_used, 1) - 1).bit_length())
        return ('random', rnd.randrange(1 << 30), rnd.randint(min(15, need + 1), 15))
    return p


def random_blocks(rnd, nblocks, limit, sizes):
    """nblocks Blocks of mixed kinds and policies; sizes(): the output bytes a block should add"""
    blocks, pos = [], 0
    for _ in range(nblocks):
        kind = rnd.choice(['stored', 'fixed', 'dynamic', 'dynamic', 'dynamic'])
        want = sizes()
        if kind == 'stored':
            toks, pos = text_tokens(rnd, pos, min(want, 3000), limit, no_match=True)
            blocks.append(Block('stored', toks))
            continue
        shape = rnd.random()
        single = no_match = None
        dist = None
        if kind == 'dynamic' and shape < 0.12:
            no_match, dist = True, 'none'
        elif kind == 'dynamic' and shape < 0.27 and pos > 0:
            single = rnd.choice([s for s in range(30) if DBASE[s] <= pos])
            dist = 'single'
        toks, pos = text_tokens(rnd, pos, want, limit, single_dsym=single, no_match=bool(no_match))
        if dist == 'single' and not any(not isinstance(t, int) for t in toks): dist = 'none'
        nl = len({t if isinstance(t, int) else length_symbol(t[0])[0] for t in toks}) + 1
        nd = len({distance_symbol(t[1])[0] for t in toks if not isinstance(t, int)})
        blocks.append(Block(kind, toks, lit=random_policy(rnd, nl), dist=dist or random_policy(rnd, nd),
                            hlit=rnd.choice(['trim', 'trim', 'max']), hdist=rnd.choice(['trim', 'trim', 'max']),
                            hclen=rnd.choice(['trim', 'trim', 'max']), rle=rnd.choice(['none', 'greedy', 'greedy', 'random', 'random']),
                            rle_seed=rnd.randrange(1 << 30), alt258=rnd.random() < 0.3))
    return blocks


def literals(rnd, n, alphabet=b'ACGTN@+\nI#'):
    return [alphabet[rnd.randrange(len(alphabet))] for _ in range(n)]


def zlib_raw(data, flush_every=None, mode=zlib.Z_PARTIAL_FLUSH, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    out = []
    step = flush_every or len(data) or 1
    for i in range(0, len(data), step):
        out.append(c.compress(data[i:i + step]))
        if flush_every: out.append(c.flush(mode))
    out.append(c.flush())
    return b''.join(out)


# ------------------------------------------------------------------ the members
def _fill(rnd, n):
    """tokens for exactly n bytes of text from position 0 (literals and short matches)"""
    return text_tokens(rnd, 0, n, n)[0]


@functools.lru_cache(maxsize=None)
def crafted_members():
    """(name, raw deflate, data): valid members of at most 65 536 bytes of output"""
    rnd = random.Random(20261017)
    out = []

    def case(name, blocks):
        raw, data = deflate(blocks)
        assert len(data) <= MAX_MEMBER, name
        out.append((name, raw, data))
        return raw, data

    head = _fill(rnd, WINDOW)
    # every extra-bit pattern's end of distance symbol 29 (24 577 ... 32 768), from positions where it just fits
    toks = list(head)
    pos = WINDOW
    for d in (24577, 32506, 32507, 32767, 32768, 32768, 32767, 32760, 32513):
        toks.append((rnd.choice([3, 4, 258]), d)); pos += toks[-1][0]
    case('dist_sym29_last_extra_bits', [Block('dynamic', toks)])
    case('dist_32768_to_position_0', [Block('dynamic', head), Block('fixed', [(258, 32768), (3, 32768), (258, 32768)])])
    body = head + text_tokens(rnd, WINDOW, 20000, MAX_MEMBER)[0]
    w = Writer().add(Block('dynamic', body, lit='deep', dist='huffman'), final=True)
    assert max(w.log[0]['llens']) == 15 and sorted(set(w.log[0]['llens']))[-2] == 14
    out.append(('lit_codes_to_15_bits',) + w.finish())
    case('lit_codes_15_bits_frequent', [Block('dynamic', body[:9000], lit='deep_rev', dist='huffman')])
    w = Writer().add(Block('dynamic', body, lit='huffman', dist='deep'), final=True)
    assert set(range(9, 16)) <= set(w.log[0]['dlens'])
    out.append(('dist_codes_to_15_bits',) + w.finish())
    case('both_codes_deep', [Block('dynamic', body[:9000], lit='deep_rev', dist='deep_rev'), Block('dynamic', body[9000:], lit='deep', dist='deep')])
    case('len_258_as_284_31', [Block('fixed', [65, (258, 1), 67, (258, 2)], alt258=True),
                               Block('dynamic', [71, (258, 1), (258, 300), (257, 3)], alt258=True)])
    case('dist_single_one_bit_code', [Block('dynamic', literals(rnd, 50) + [(10, 40), (258, 33), (3, 48)], dist='single')])
    case('dist_none_literal_only', [Block('dynamic', literals(rnd, 500), dist='none')])
    case('lit_only_end_of_block', [Block('dynamic', [], lit='single', dist='none'), Block('fixed', literals(rnd, 20)),
                                   Block('dynamic', [], lit='single', dist='none')])
    # HCLEN 5: the code-length code has 0 and 8 only, so 256 literal/length codes of 8 bits; HLIT 257, HDIST 1 (no distance code)
    w = Writer().add(Block('dynamic', [1 + rnd.randrange(255) for _ in range(600)], lit=[0] + [8] * 256, dist='none', rle='none'), final=True)
    assert (w.log[0]['hlit'], w.log[0]['hdist'], w.log[0]['hclen']) == (257, 1, 5)
    out.append(('hlit_257_hdist_1_hclen_5',) + w.finish())
    w = Writer().add(Block('dynamic', body[:3000], hlit='max', hdist='max', hclen='max'), final=True)
    assert (w.log[0]['hlit'], w.log[0]['hdist'], w.log[0]['hclen']) == (286, 30, 19)
    out.append(('hlit_286_hdist_30_hclen_19',) + w.finish())
    # header run-lengths
    few = literals(rnd, 300, b'ACGT') + [(258, 7), (3, 1)]
    for mode, pair in (('zero16_17', (17, 16)), ('zero16_18', (18, 16))):
        w = Writer().add(Block('dynamic', few, rle=mode), final=True)
        ops = [s for s, _ in w.log[0]['ops']]
        assert any(ops[i:i + 2] == list(pair) for i in range(len(ops)))
        out.append(('rle_16_after_%d' % pair[0],) + w.finish())
    w = Writer().add(Block('dynamic', few), final=True)
    assert (18, 127) in w.log[0]['ops']
    out.append(('rle_18_with_138',) + w.finish())
    # 260 literal/length lengths: ... 256: 2, 257 - 259: 4 4 4 (a 16-run that ends at HLIT), then the distance lengths 1 1 / 4 4
    lit_lens = [0] * 65 + [2] + [0] * 5 + [2] + [0] * 184 + [2] + [4, 4, 4, 4]
    toks = [65, 71, 65, (4, 1), (5, 2), (6, 2), (3, 2)]
    for name, dl in (('rle_run_ends_at_hlit', [1, 1]), ('rle_run_crosses_hlit', [4] * 16)):
        w = Writer().add(Block('dynamic', toks, lit=lit_lens, dist=dl), final=True)
        ops, n = w.log[0]['ops'], 0
        ends = []
        for s, e in ops:
            n += len(replay_ops([(4, 0), (s, e)])) - 1 if s == 16 else len(replay_ops([(s, e)]))
            ends.append((s, n))
        assert w.log[0]['hlit'] == 261
        if name == 'rle_run_ends_at_hlit': assert (16, 261) in ends
        else: assert any(s == 16 and a < 261 < b for (_, a), (s, b) in zip(ends, ends[1:]))
        out.append((name,) + w.finish())
    case('empty_blocks_of_every_type', [Block('stored'), Block('fixed'), Block('fixed'), Block('fixed'), Block('dynamic', lit='single', dist='none'),
                                        Block('dynamic', lit=[0] * 256 + [1, 1], dist='none'), Block('stored'), Block('stored'),
                                        Block('fixed', literals(rnd, 9)), Block('fixed'), Block('dynamic', lit='single', dist='none'), Block('fixed')])
    data = bytes(literals(rnd, 30000))
    out.append(('zlib_partial_flush',) + checked(zlib_raw(data, 1500), data))
    for k in range(8):
        # a fixed block of 10 + 9 b bits (b long literals) puts the next header at bit (2 + b) % 8
        lead = Block('fixed', [200 + j for j in range((k - 2) % 8)])
        w = Writer().add(lead)
        assert w.bits.n % 8 == k
        w.add(Block('stored', literals(rnd, 100))).add(Block('fixed', [(20, 50), 66])).add(lead)
        w.add(Block('stored', literals(rnd, 7)), final=True)
        out.append(('stored_header_at_bit_%d' % k,) + w.finish())
    case('stored_len_0_final', [Block('dynamic', body[:2000]), Block('stored')])
    case('stored_len_65535', [Block('stored', literals(rnd, 65535)), Block('fixed', [66])])
    case('stored_last_after_huffman', [Block('dynamic', body[:2000]), Block('fixed', [(258, 1000)]), Block('stored', literals(rnd, 333))])
    toks, pos = text_tokens(rnd, 0, 65278, 65278)
    assert pos == 65278
    case('out_65536_ends_in_match_258', [Block('dynamic', toks + [(258, 32768)], lit='deep')])
    case('dist_equals_pos', [Block('fixed', [65, (3, 1), (4, 4), 66, (258, 9), (258, 267)]),
                             Block('dynamic', literals(rnd, 733) + [(258, 1258)])])
    case('dist_1_len_258', [Block('fixed', [78, (258, 1), (258, 1)]), Block('dynamic', [10, (258, 1), (258, 1), (258, 1)], dist='single')])
    # seeded random members
    for i in range(200):
        r = random.Random(7000 + i)
        total = r.choice([r.randint(1, 3000), r.randint(32768, MAX_MEMBER), r.randint(33000, MAX_MEMBER), MAX_MEMBER])
        nb = r.randint(1, 6)
        case('random/%d' % i, random_blocks(r, nb, total, lambda: max(1, total // nb + r.randint(-200, 200))))
    return out


# ------------------------------------------------------------------ the streams (gzip files)
def _front(rnd, n=40000):
    """A stored block of n random bytes: a member's first chunks, with no unit inside for the finder"""
    return Block('stored', bytes(rnd.getrandbits(8) for _ in range(n)))


def _quiet(rnd, n):
    """tokens for n symbols that copy nothing from before them: a literal, then matches at distance 1 (two bits each under Huffman)"""
    toks, left = [], n
    while left:
        toks.append(rnd.choice(b'ACGT')); left -= 1
        if left >= 3:
            l = min(258, left)
            toks.append((l, 1)); left -= l
    return toks


def _span(toks):
    return sum(1 if isinstance(t, int) else t[0] for t in toks)


def _member_ending_at(rnd, target):
    """A gzip member whose deflate data ends on the last bit of file byte target - 1 (its trailer starts at `target`)"""
    w = Writer().add(Block('dynamic', _fill(rnd, 3000)))
    w.add(Block('stored', literals(rnd, 50)))
    last = Block('dynamic', [(258, 1000), 65, 66, (30, 2)])
    probe = Writer(); probe.out = bytearray(w.out); probe.add(last, final=True)
    gap = 8 * (target - len(GZIP_HEADER)) - w.bits.n - probe.bits.n
    for blk in filler(gap): w.add(blk)
    w.add(last, final=True)
    assert w.bits.n == 8 * (target - len(GZIP_HEADER))
    return gzip_wrap(*w.finish()), bytes(w.out)


@functools.lru_cache(maxsize=None)
def crafted_streams():
    """(name, gzip file, data): valid gzip files that are not BGZF, each of at most about 300 KB of output"""
    rnd = random.Random(20261018)
    out = []

    def case(name, blocks):
        raw, data = deflate(blocks)
        out.append((name, gzip_wrap(raw, data), data))
        return out[-1][1:]

    # a chunk that starts at the dynamic block after the front reads its window through markers
    case('marker_oldest_ring_entry', [_front(rnd), Block('dynamic', [(3, 32768), 65, (258, 32768), (200, 32767)] + literals(rnd, 300)),
                                     Block('dynamic', [(258, 32768)] * 3 + literals(rnd, 100) + [(258, 32768)])])
    toks = [(258, 32768), (258, 32700), (258, 32600)] + _quiet(rnd, 32000)
    toks += [(258, 32768), (258, 32767 - 100), (258, 32768 - 257), (258, 32768)]            # sources across the ring's end, in and out of markers
    case('source_wraps_the_ring', [_front(rnd), Block('dynamic', toks + _quiet(rnd, 33000) + [(258, 32768), (258, 32600)])])
    case('all_matches_at_32768', [Block('dynamic', _fill(rnd, WINDOW)), Block('dynamic', [(258, 32768)] * 300 + [(3, 32768)]),
                                  Block('dynamic', [(257, 32768), (4, 32768)] * 300, dist='single', lit='deep')])
    case('overlapping_match_of_markers', [_front(rnd), Block('dynamic', [(258, 3), (258, 1), 65, (100, 70), (258, 64), (258, 65), (200, 63)]
                                                             + literals(rnd, 50) + [(258, 600), (258, 2)])] +
         [Block('dynamic', [(258, 5 + k), (30, 3), 67, (258, 1)] + literals(rnd, 700)) for k in range(30)])
    # ten markers copied on every 30 000 symbols: the chunk stays u16 for seven windows, then 40 000 quiet symbols let it switch
    toks = [(10, 30000)]
    for _ in range(7): toks += _quiet(rnd, 29990) + [(10, 30000)]
    case('marker_chain_250k', [_front(rnd), Block('dynamic', toks + _quiet(rnd, 40000))])
    # the switch test runs when the ring flushes: at symbol 32 768 + 4 096 j.  Markers up to symbol 4 096 exactly -> the test at 36 864 is
    # lastm + 32 768 == pos; one symbol more and it has to wait for the next flush.  The token at 36 864 then copies symbol 4 096, the
    # oldest ring entry: the first byte after the markers in the one case, the last marker in the other, which a switch one symbol
    # early would cut to a byte
    for name, last in (('switch_at_exactly_32768', 226), ('switch_one_symbol_late', 227)):
        toks = [(258, 32768)] * 15 + [(last, 32768)]
        assert _span(toks) == 3870 + last                    # symbols 0 ... 3 869 + last are markers
        quiet = _quiet(rnd, 36864 - 3870 - last)
        assert _span(toks + quiet) == 36864                  # a token starts at 36 864: the second flush sees pos = 36 864
        case(name, [_front(rnd), Block('dynamic', toks + quiet + [(3, 32768)] + _quiet(rnd, 12000))])
    toks = [(100, 32768)] + _quiet(rnd, 32768)
    case('chunk_ends_at_exactly_32768', [_front(rnd), Block('dynamic', toks)])                # the final flush at lastm + 32 768 == len
    fixed = []
    pos = 0
    while pos < 200000:
        t, pos = text_tokens(rnd, pos, 4000, 200000)
        fixed.append(Block('fixed', t, alt258=len(fixed) % 2 == 1))
    case('fixed_only_200k', fixed)
    empty = Block('dynamic', lit='single', dist='none')
    case('empty_dynamic_blocks_x64', [Block('dynamic', _fill(rnd, 5000))] + [empty] * 64 + [Block('dynamic', [(258, 5000), 66])] + [empty] * 3)
    data = bytes(literals(rnd, 120000))
    out.append(('zlib_partial_flush', gzip_wrap(zlib_raw(data, 2500), data), data))
    # units at chunk boundaries: a dynamic header at bit 8 * 16 384, a stored block's LEN at byte 16 384 (file offsets)
    for name, blk, off in (('dynamic_unit_at_chunk_boundary', Block('dynamic', [(258, 32768), 65] + _fill(rnd, 4000)[1:]), 0),
                           ('stored_unit_at_chunk_boundary', Block('stored', literals(rnd, 500)), 8)):
        w = Writer().add(_front(rnd, 10000))
        # a stored unit's position is its LEN field, one byte after a header at bit 0 of the byte before
        gap = 8 * (16384 - len(GZIP_HEADER)) - off - w.bits.n
        for f in filler(gap): w.add(f)
        assert 8 * len(GZIP_HEADER) + w.bits.n + off == 8 * 16384
        if name.startswith('dynamic'):
            w.add(Block('dynamic', _quiet(rnd, 30000))); gap = 8 * (3 * 16384 - len(GZIP_HEADER)) - w.bits.n
            for f in filler(gap): w.add(f)
        w.add(blk).add(Block('dynamic', [(258, 10000), (258, 1)] + literals(rnd, 2000)), final=True)
        raw, data = w.finish()
        out.append((name, gzip_wrap(raw, data), data))
    parts = []
    for name, target in (('member_ends_at_chunk_16384', 16384), ('member_ends_at_chunk_6000', 6000)):
        blob, data = _member_ending_at(rnd, target)
        assert len(blob) == target + 8
        more = bytes(literals(rnd, 5000))
        out.append((name, blob + gzip.compress(more, mtime=0), data + more))
        parts.append((blob, data))
    # several members: crafted ones beside gzip.compress's and an empty one
    named = {n: (b, d) for n, b, d in out}
    big = bytes(literals(rnd, 30000))
    mix = [named['all_matches_at_32768'], (gzip.compress(more, mtime=0), more), (gzip.compress(b'', mtime=0), b''), named['overlapping_match_of_markers'],
           parts[1], named['empty_dynamic_blocks_x64'], (gzip.compress(big, 1, mtime=0), big)]
    out.append(('multi_member_mix', b''.join(b for b, _ in mix), b''.join(d for _, d in mix)))
    mix = [(gzip.compress(b'', mtime=0), b''), named['marker_oldest_ring_entry'], named['fixed_only_200k'], (gzip.compress(b'', mtime=0), b'')]
    out.append(('multi_member_fixed_and_markers', b''.join(b for b, _ in mix), b''.join(d for _, d in mix)))
    for i in range(40):
        r = random.Random(9000 + i)
        nb = r.randint(20, 200)
        total = r.randint(60000, 300000)
        case('random/%d' % i, random_blocks(r, nb, total, lambda: max(1, total // nb + r.randint(-300, 300))))
    return out


# ------------------------------------------------------------------ text as crafted blocks
def tokenize(text, prefer=(WINDOW,)):
    """Greedy tokens of `text`: a match at one of the preferred distances wherever three bytes agree there, else at the last place the next
    three bytes were seen, else a literal"""
    toks, pos, n, last = [], 0, len(text), {}
    while pos < n:
        key = text[pos:pos + 3]
        step = 1
        if len(key) == 3:
            for d in prefer + ((pos - last[key],) if key in last else ()):
                if 0 < d <= min(pos, WINDOW) and text[pos - d:pos - d + 3] == key:
                    l = 3
                    while l < 258 and pos + l < n and text[pos + l - d] == text[pos + l]: l += 1
                    toks.append((l, d)); step = l
                    break
        if step == 1: toks.append(text[pos])
        for q in range(pos, min(pos + step, n - 2)): last[text[q:q + 3]] = q
        pos += step
    return toks


def crafted_text_members(text, kind, member=49152, per_block=1500):
    """[(raw deflate, data)] of `text` cut into members of `member` bytes, each tokenised into blocks of per_block tokens.  kind 'deep':
    dynamic blocks with comb codes (15-bit codes) and matches at distance 32 768; 'fixed': fixed blocks only."""
    out = []
    for i in range(0, len(text), member):
        piece = text[i:i + member]
        toks = tokenize(piece)
        cuts = [toks[k:k + per_block] for k in range(0, len(toks), per_block)]
        if kind == 'deep':
            blocks = [Block('dynamic', c, lit='deep', dist='deep', alt258=k % 2 == 1) for k, c in enumerate(cuts)]
            if len(piece) > WINDOW + 3000: assert any(t[1] == WINDOW for t in toks if not isinstance(t, int))
        else:
            blocks = [Block('fixed', c) for c in cuts]
        w = Writer()
        for k, blk in enumerate(blocks): w.add(blk, final=k == len(blocks) - 1)
        if kind == 'deep': assert all(max(e['llens']) == 15 and max(e['dlens']) == 15 for e in w.log)
        raw, data = w.finish()
        assert data == piece
        out.append((raw, data))
    return out


# ------------------------------------------------------------------ invalid neighbours
def _dyn_header(b, hlit, hdist, clens, ops, hclen=19):
    """A dynamic block header (BFINAL = 1) written as given, valid or not"""
    b.put(1, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
    for s in ORDER[:hclen]: b.put(clens.get(s, 0), 3)
    cc = canonical_codes([clens.get(s, 0) for s in range(19)])
    for sym, extra in ops:
        b.code(*cc[sym])
        if sym >= 16: b.put(extra, {16: 2, 17: 3, 18: 7}[sym])
    return b


def behind_valid_front(raw):
    """A gzip member of a stored block, a dynamic block and then the bits of `raw` (an invalid block whose fault does not depend on the
    output before it): with small chunks a speculative chunk starts at the dynamic block and meets the fault"""
    rnd = random.Random(99)
    w = Writer().add(_front(rnd, 3000)).add(Block('dynamic', text_tokens(rnd, 3000, 2000, 5000)[0]))
    for byte in raw: w.bits.put(byte, 8)
    blob = GZIP_HEADER + w.bits.bytes() + bytes(8)
    try:
        zlib.decompress(blob, 31)
    except zlib.error:
        return blob
    raise AssertionError('zlib accepts the stream')


def zlib_refuses(raw, isize):
    """Does zlib refuse the stream as a gzip member of `isize` bytes (its CRC-32 taken from whatever zlib makes of the stream)?"""
    d = zlib.decompressobj(-15)
    try:
        got = d.decompress(raw) + d.flush()
    except zlib.error:
        return True
    if not d.eof:
        return True
    try:
        zlib.decompressobj(31).decompress(GZIP_HEADER + raw + struct.pack('<II', zlib.crc32(got[:isize]), isize))
    except zlib.error:
        return True
    return False


@functools.lru_cache(maxsize=None)
def crafted_invalid():
    """(name, raw deflate, isize, status of inflate_core.h): the nearest invalid neighbours of the valid edges; zlib refuses each"""
    out = []
    b = Bits().put(1, 1).put(1, 2)
    for s in (65, 66, 67): fixed_lit(b, s)
    fixed_lit(b, 257); b.code(3, 5); fixed_lit(b, 256)                                        # length 3, distance 4 at position 3
    out.append(('dist_equals_pos_plus_1', b.bytes(), 6, 7))
    # 285 / 284 + 31 at position 65 279 would end at 65 537
    rnd = random.Random(5)
    toks, pos = text_tokens(rnd, 0, 65279, 65279)
    w = Writer().add(Block('dynamic', toks + [(258, 32768)]), final=True)
    out.append(('match_258_ends_at_65537', w.bits.bytes(), 65536, 8))
    # distance symbols 30 / 31 cannot be in a dynamic code: HDIST 31 and 32 are refused by their count
    eight = {8: 1, 18: 2, 0: 2}
    for hdist in (31, 32):
        b = _dyn_header(Bits(), 257, hdist, eight, [(8, 0)] * 256 + [(8, 0)] + [(0, 0)] * hdist)
        out.append(('hdist_%d' % hdist, b.put(0, 32).bytes(), 0, 11))
    zeros = lambda n: [(18, 127)] * (n // 138) + ([(18, n % 138 - 11)] if n % 138 >= 11 else [(0, 0)] * (n % 138))
    cl = {0: 2, 2: 2, 1: 2, 18: 2}
    b = _dyn_header(Bits(), 257, 1, cl, zeros(255) + [(2, 0), (2, 0), (0, 0)])                # two codes of 2 bits: 255, 256
    out.append(('incomplete_literal_code_of_two', b.put(0, 32).bytes(), 0, 4))
    b = _dyn_header(Bits(), 257, 1, cl, zeros(255) + [(1, 0), (1, 0), (2, 0)])                # literal code complete, one distance code of 2 bits
    out.append(('distance_code_single_two_bits', b.put(0, 32).bytes(), 0, 4))
    b = _dyn_header(Bits(), 257, 1, {0: 2, 1: 2, 18: 2}, zeros(255) + [(1, 0), (1, 0), (0, 0)])
    out.append(('incomplete_code_length_code', b.put(0, 32).bytes(), 0, 4))
    b = _dyn_header(Bits(), 257, 1, {18: 1}, zeros(258))                                       # one code of one bit is not enough for zlib here
    out.append(('code_length_code_single_one_bit', b.put(0, 32).bytes(), 0, 4))
    cl16 = {0: 2, 1: 2, 16: 2, 18: 2}
    b = _dyn_header(Bits(), 257, 1, cl16, [(16, 0)] + zeros(252) + [(1, 0), (1, 0), (0, 0)])
    out.append(('repeat_as_first_length', b.put(0, 32).bytes(), 0, 5))
    b = _dyn_header(Bits(), 257, 1, cl16, zeros(255) + [(1, 0), (1, 0), (16, 0)])              # 3 more lengths where 1 is left
    out.append(('run_overshoots_hlit_plus_hdist', b.put(0, 32).bytes(), 0, 5))
    b = _dyn_header(Bits(), 257, 1, cl16, zeros(254) + [(1, 0), (1, 0), (0, 0), (18, 0)])
    out.append(('zero_run_overshoots_hlit_plus_hdist', b.put(0, 32).bytes(), 0, 5))
    b = _dyn_header(Bits(), 257, 1, cl, zeros(254) + [(1, 0), (1, 0), (0, 0), (0, 0)])         # literals 254, 255; no 256
    out.append(('no_end_of_block_code', b.put(0, 32).bytes(), 0, 4))
    b = _dyn_header(Bits(), 257, 1, {18: 1, 0: 1}, zeros(258), hclen=4)                        # 16, 17, 18 and 0 only: nothing but zero lengths
    out.append(('hclen_4_only_zero_lengths', b.put(0, 64).bytes(), 0, 4))
    # a code-length code of one one-bit code, or of none, is refused as such by both decoders, whatever follows it
    b = _dyn_header(Bits(), 257, 1, {16: 1}, [(16, 0)])
    out.append(('precode_only_16_then_16', b.put(0, 32).bytes(), 0, 4))
    b = _dyn_header(Bits(), 257, 1, {8: 1}, [])
    out.append(('precode_only_8_then_ones', b.put(0xFFFFFFFF, 32).put(0xFFFFFFFF, 32).bytes(), 0, 4))
    b = _dyn_header(Bits(), 257, 1, {0: 1}, [])
    out.append(('precode_only_0_then_zeros', b.put(0, 64).bytes(), 0, 4))
    b = _dyn_header(Bits(), 257, 1, {}, [], hclen=4)
    out.append(('precode_hclen_4_all_zero', b.put(0, 64).bytes(), 0, 4))
    for name, raw, isize, _ in out:
        assert zlib_refuses(raw, isize), name
    return out
