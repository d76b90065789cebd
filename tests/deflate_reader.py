"""A plain raw-deflate reader (RFC 1951) for the tests of the compressor, and two exact references for its code builder.

The reader goes bit by bit and keeps everything a test may want to look at: for every block BTYPE, HLIT, HDIST and HCLEN, the
code-length-code lengths as written, the code-length symbols with their extra bits, both sets of code lengths and the tokens (an int is
a literal, a pair is (length, distance)).  Like zlib it refuses a code that is over-subscribed or incomplete; the two incomplete codes
zlib lets pass (a literal/length or distance code of one 1-bit code, and a code of no lengths at all, which fails only when it is
used) pass here too.  It is slow and does not care.

The references, in exact integers:
  huffman_depths / unlimited_depth   the unconstrained Huffman tree of a histogram under the compressor's tie rule (symbols sorted by
                                     (weight, symbol), a leaf before an internal node of the same weight), so that "deeper than the
                                     limit" means the same here and in uq_def_huffman
  package_merge_cost                 the least sum of frequency x length of a prefix code whose lengths are at most `limit`
                                     (Larmore and Hirschberg's package-merge), brute_force_cost the same by enumeration
"""
import itertools
import struct
import zlib

from deflate_writer import DBASE, DEXT, LBASE, LEXT, ORDER, distance_symbol, length_symbol

CL_EXTRA = {16: 2, 17: 3, 18: 7}
CL_BASE = {16: 3, 17: 3, 18: 11}


class DeflateError(ValueError):
    pass


class BitReader:
    def __init__(self, data, bit=0):
        self.data, self.pos = bytes(data), bit

    def bit(self):
        if self.pos >= 8 * len(self.data): raise DeflateError('the stream ends inside a block')
        v = (self.data[self.pos >> 3] >> (self.pos & 7)) & 1
        self.pos += 1
        return v

    def bits(self, n):                                      # least significant bit first
        v = 0
        for k in range(n): v |= self.bit() << k
        return v


class Code:
    """The canonical code of a list of lengths (RFC 1951 3.2.2).  kind: 'codelen', 'litlen' or 'dist'."""

    def __init__(self, lens, kind):
        self.kind = kind
        self.maxlen = max(lens) if lens else 0
        count = [0] * (self.maxlen + 2)
        for l in lens: count[l] += 1
        count[0] = 0
        left = 1                                            # zlib's inflate_table: the code space left, doubling per bit
        for l in range(1, self.maxlen + 1):
            left = 2 * left - count[l]
            if left < 0: raise DeflateError('over-subscribed %s code' % kind)
        if self.maxlen and left > 0 and (kind == 'codelen' or self.maxlen != 1):
            raise DeflateError('incomplete %s code' % kind)
        self.table, code = {}, 0
        nxt = [0] * (self.maxlen + 2)
        for l in range(1, self.maxlen + 1):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        for s, l in enumerate(lens):
            if l:
                self.table[(l, nxt[l])] = s
                nxt[l] += 1

    def read(self, br):
        code = 0
        for l in range(1, self.maxlen + 1):
            code = (code << 1) | br.bit()                   # Huffman codes come most significant bit first
            s = self.table.get((l, code))
            if s is not None: return s
        raise DeflateError('a %s code that the block does not have' % self.kind)


FIXED_LLENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DLENS = [5] * 32                                      # 30 and 31 take code space and are never valid


def _read_dynamic_header(br, blk):
    hlit, hdist, hclen = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
    if hlit > 286 or hdist > 30: raise DeflateError('too many length or distance symbols')
    written = [br.bits(3) for _ in range(hclen)]
    clens = [0] * 19
    for k, l in enumerate(written): clens[ORDER[k]] = l
    ccode = Code(clens, 'codelen')
    lens, syms = [], []
    while len(lens) < hlit + hdist:
        s = ccode.read(br)
        if s < 16:
            syms.append((s, 0)); lens.append(s)
            continue
        ex = br.bits(CL_EXTRA[s])
        syms.append((s, ex))
        n = CL_BASE[s] + ex
        if s == 16:
            if not lens: raise DeflateError('a repeat with no length before it')
            lens += [lens[-1]] * n
        else:
            lens += [0] * n
        if len(lens) > hlit + hdist: raise DeflateError('a run past the last code length')
    blk.update(hlit=hlit, hdist=hdist, hclen=hclen, clens_written=written, clens=clens, cl_syms=syms, llens=lens[:hlit], dlens=lens[hlit:])
    if not blk['llens'][256]: raise DeflateError('no end-of-block code')


def inflate(raw, bit=0):
    """(the inflated bytes, the list of blocks, the bit after the final block) of the raw deflate stream that starts at `bit` of raw."""
    br = BitReader(raw, bit)
    out, blocks = bytearray(), []
    while True:
        final, btype = br.bit(), br.bits(2)
        blk = dict(final=final, btype=btype, first_bit=br.pos - 3, start=len(out), tokens=[])
        blocks.append(blk)
        if btype == 0:
            br.pos = (br.pos + 7) & ~7
            n, nn = br.bits(16), br.bits(16)
            if n ^ nn != 0xFFFF: raise DeflateError('stored block: LEN and NLEN disagree')
            at = br.pos >> 3
            if at + n > len(br.data): raise DeflateError('the stream ends inside a stored block')
            blk['stored'] = br.data[at:at + n]
            out += blk['stored']
            br.pos += 8 * n
        elif btype == 3:
            raise DeflateError('block type 3')
        else:
            if btype == 2:
                _read_dynamic_header(br, blk)
            else:
                blk.update(llens=list(FIXED_LLENS), dlens=list(FIXED_DLENS))
            lcode, dcode = Code(blk['llens'], 'litlen'), Code(blk['dlens'], 'dist')
            while True:
                s = lcode.read(br)
                if s < 256:
                    blk['tokens'].append(s); out.append(s)
                    continue
                if s == 256: break
                if s > 285: raise DeflateError('length symbol %d' % s)
                length = LBASE[s - 257] + br.bits(LEXT[s - 257])
                d = dcode.read(br)
                if d > 29: raise DeflateError('distance symbol %d' % d)
                dist = DBASE[d] + br.bits(DEXT[d])
                if dist > len(out): raise DeflateError('a distance before the start of the output')
                blk['tokens'].append((length, dist))
                for _ in range(length): out.append(out[-dist])
        blk['end_bit'] = br.pos
        if final: return bytes(out), blocks, br.pos


def read_member(m):
    """(data, blocks) of one gzip / BGZF member that fills `m` exactly: header, CRC-32 and ISIZE checked."""
    if m[:3] != b'\x1f\x8b\x08': raise DeflateError('not a gzip member')
    at = 10
    if m[3] & 4: at += 2 + struct.unpack('<H', m[10:12])[0]
    if m[3] & ~4: raise DeflateError('gzip flags the reader does not know')
    data, blocks, end = inflate(m[at:])
    tail = at + (end + 7) // 8
    if len(m) != tail + 8: raise DeflateError('the member does not end with its trailer')
    crc, isize = struct.unpack('<II', m[tail:])
    if crc != zlib.crc32(data) or isize != len(data): raise DeflateError('CRC-32 or ISIZE')
    return data, blocks


def histograms(blk):
    """(literal/length counts [286], distance counts [30]) of a block's tokens, the end-of-block symbol counted once; a length of 258 is
    symbol 285, as the compressor writes it."""
    lf, df = [0] * 286, [0] * 30
    for t in blk['tokens']:
        if isinstance(t, tuple):
            lf[length_symbol(t[0])[0]] += 1
            df[distance_symbol(t[1])[0]] += 1
        else:
            lf[t] += 1
    lf[256] += 1
    return lf, df


def codelen_histogram(blk):
    cf = [0] * 19
    for s, _ in blk['cl_syms']: cf[s] += 1
    return cf


def run_spans(blk):
    """[(code-length symbol, extra bits' value, first index, count)] over the hlit + hdist sequence of a dynamic block."""
    out, i = [], 0
    for s, ex in blk['cl_syms']:
        n = 1 if s < 16 else CL_BASE[s] + ex
        out.append((s, ex, i, n))
        i += n
    return out


# ------------------------------------------------------------------ the references
def huffman_depths(freq):
    """{symbol: depth} of the unconstrained Huffman tree over the symbols with a weight, built as uq_def_huffman builds it: leaves sorted by
    (weight, symbol), the two least of (next leaf, next internal node) merged, a leaf before an internal node of the same weight.  One
    symbol alone gets depth 1, as the format needs one bit."""
    leaves = sorted((f, s) for s, f in enumerate(freq) if f)
    m = len(leaves)
    if m == 0: return {}
    if m == 1: return {leaves[0][1]: 1}
    weight = [f for f, _ in leaves]
    parent = [None] * (2 * m - 1)
    li, ni = 0, m
    for k in range(m, 2 * m - 1):
        pick = []
        for _ in range(2):
            if li < m and (ni >= k or weight[li] <= weight[ni]):
                pick.append(li); li += 1
            else:
                pick.append(ni); ni += 1
        weight.append(weight[pick[0]] + weight[pick[1]])
        parent[pick[0]] = parent[pick[1]] = k
    depth = [0] * (2 * m - 1)
    for k in range(2 * m - 3, -1, -1): depth[k] = depth[parent[k]] + 1
    return {leaves[i][1]: depth[i] for i in range(m)}


def unlimited_depth(freq):
    d = huffman_depths(freq)
    return max(d.values()) if d else 0


def package_merge_cost(freq, limit):
    """The least sum of freq[s] x len[s] over prefix codes of the weighted symbols with every length in 1..limit."""
    w = sorted(f for f in freq if f)
    m = len(w)
    if m == 0: return 0
    if m == 1: return w[0]                                  # one bit: the format has no code of no bits
    assert m <= 1 << limit, 'no code that short'
    items = list(w)                                         # the items of width 2^-limit
    for _ in range(limit - 1):
        packages = [items[2 * i] + items[2 * i + 1] for i in range(len(items) // 2)]
        items = sorted(w + packages)
    return sum(items[:2 * m - 2])


def brute_force_cost(freq, limit):
    """package_merge_cost by trying every assignment of lengths that satisfies Kraft's inequality (small alphabets only)."""
    w = [f for f in freq if f]
    if len(w) < 2: return sum(w)
    best = None
    for lens in itertools.product(range(1, limit + 1), repeat=len(w)):
        if sum(1 << (limit - l) for l in lens) <= 1 << limit:
            c = sum(f * l for f, l in zip(w, lens))
            if best is None or c < best: best = c
    return best


def code_cost(freq, lens):
    return sum(f * l for f, l in zip(freq, lens))


def kraft_units(lens, limit):
    """sum of 2^-l over the nonzero lengths, in units of 2^-limit: 1 << limit is a complete code"""
    return sum(1 << (limit - l) for l in lens if l)
