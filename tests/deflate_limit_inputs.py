"""Blocks that drive the deflate compressor's code builder (uq_def_huffman) past its length limits, and a family of small blocks for the
shapes of the dynamic header.  Nothing is stored: every block is generated from the parameters below, and its name says which path it is
built to reach.  tests/test_deflate_limits_cpu.py proves for every block, at both levels, that the path is taken.

lit15, clen7 (filler_block): `k` payload byte values with the counts 1, 1, 2, 3, 5, ... (a Fibonacci histogram makes the deepest Huffman
tree), shuffled, and after every payload byte `per` filler bytes drawn from `nfill` other values, so that hardly any four bytes repeat
and the matcher leaves the histogram alone.  The parameters kept are the winners of a seeded search over this recipe through
ops.bgzf_block_host and the reader's histograms (k 15..22, nfill 3..215, per 1..3, two seeds each, cut at 65 280 bytes or shorter).

dist15 (planted_block): the distance histogram cannot be written into the text, it has to be found by the matcher; the generator plants
copies where the matcher's own rule finds them.

hdr/... (header_blocks): texts of at most 512 bytes in which no byte repeats within two positions have no match at either level, so their
literal counts are exact; hdr/run_crosses_hlit needs exact match counts and is planted the same way as dist15.
"""
import functools
import random

from deflate_writer import DBASE

BLOCK = 65280
ROUND = 512                                                 # UQ_DEF_ROUND: level 1 sees only positions from before the current round
HASH_BITS = 12


def fib(k):
    a = [1, 1]
    while len(a) < k: a.append(a[-1] + a[-2])
    return a[:k]


def filler_block(seed, k, nfill, per, base=0, n=BLOCK):
    rnd = random.Random(seed)
    values = [(base + 3 * i) % 256 for i in range(k)]
    pay = [v for v, c in zip(values, fib(k)) for _ in range(c)]
    rnd.shuffle(pay)
    fillers = rnd.sample([x for x in range(256) if x not in set(values)], nfill)
    out = bytearray()
    for p in pay:
        out.append(p)
        for _ in range(per): out.append(rnd.choice(fillers))
    return bytes(out[:n])


# ------------------------------------------------------------------ planted matches: the distance code
DLAST = DBASE[1:] + [32769]                                 # symbol s covers DBASE[s] .. DLAST[s] - 1


def _hash(b, p):
    v = b[p] | (b[p + 1] << 8) | (b[p + 2] << 16) | (b[p + 3] << 24)
    return ((v * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def planted_block(seed, plan, gap=1, n=BLOCK, fill=0, pad=True, log=None):
    """A block of random bytes with copied words planted in it: plan = [(distance symbol, match length >= 4)], each planted where the
    level-1 matcher finds it at exactly that length and at a distance of that symbol.  The matcher looks a position's four bytes up in a
    table of 4 096 hashes that holds the latest position from before the position's round of 512, so a source is taken only if it lies
    before the round and no later position before the round has its hash; the generator keeps the same table and checks every plant
    against it before it commits the bytes.  Near symbols fit only at a round's first positions, so the bytes before a round are
    filled with fresh ones while such plants wait.  `gap` fresh bytes follow every word (the first differs from the byte that would
    lengthen the match), `fill` more follow every plant; `pad`: fresh bytes up to n behind the last plant.  Returns (block, plants that did not fit)."""
    rnd = random.Random(seed)
    out = bytearray()
    table = {}                                              # hash -> positions, ascending; positions below `hashed`
    hashed = 0
    todo = sorted(plan, key=lambda sl: (DLAST[sl[0]], sl[1]))           # nearest first

    def fresh(k, avoid=None):
        for _ in range(k):
            v = rnd.getrandbits(8)
            while avoid is not None and v == avoid: v = rnd.getrandbits(8)
            out.append(v)
            avoid = None

    def commit():
        nonlocal hashed
        while hashed + 4 <= len(out):
            table.setdefault(_hash(out, hashed), []).append(hashed)
            hashed += 1

    def latest_before(h, r0):
        for q in range(min(r0, len(out) - 3) - 1, hashed - 1, -1):     # not yet in the table: the bytes just appended complete them
            if _hash(out, q) == h: return q
        for q in reversed(table.get(h, ())):
            if q < r0: return q
        return None

    def stray(q):                                           # would the matcher find three bytes at q, ahead of the plant behind it?
        c = latest_before(_hash(out, q), q - q % ROUND)
        return c is not None and out[c:c + 3] == out[q:q + 3]

    def plant(s, length):
        p = len(out)
        r0 = p - p % ROUND
        lo, hi = max(DBASE[s], p - r0 + 1), min(DLAST[s] - 1, p)
        if lo > hi: return False
        ds = list(range(lo, hi + 1))
        rnd.shuffle(ds)
        for d in ds[:400]:
            c = p - d
            for i in range(length): out.append(out[c + i])
            if latest_before(_hash(out, p), r0) == c and not any(stray(q) for q in range(max(p - 3, 0), p)):
                fresh(gap, avoid=out[c + length])
                if log is not None: log.append((p, length, d))
                return True
            del out[p:]
        return False

    while todo and len(out) + 300 < n:
        p = len(out)
        left = ROUND - p % ROUND
        for k, (s, length) in enumerate(todo):
            if plant(s, length):
                del todo[k]
                fresh(fill)
                break
        else:
            if p < ROUND: fresh(left)                       # nothing matches in the first round
            elif todo[0][0] < 8 and left <= 8 + gap: fresh(left)        # a near plant waits for the round's first positions
            else: fresh(1)
        commit()
    if pad: fresh(max(0, n - len(out)))
    return bytes(out[:n]), todo


# rarest first: the far distances (the hash table forgets them) and the nearest (a round's first positions only) get the small counts,
# 513 .. 3 072 the large ones, where also the few matches land that the plan did not plant
DIST_ORDER = [29, 28, 0, 27, 1, 26, 25, 24, 12, 16, 17, 23, 22, 21, 20, 19, 18]


def dist_counts(k=17, margin=3, per=150):
    """k counts, each more than the sum of all but the one before it: the Huffman tree over them is a chain k - 1 deep.  The margin
    (margin + sum / per) absorbs the handful of matches that level 2's extra candidates find elsewhere."""
    a = [1, 1]
    while len(a) < k: a.append(sum(a[:-1]) + 1 + margin + sum(a[:-1]) // per)
    return a


def dist_block(seed, pad=True):
    plan = [(s, 4) for s, c in zip(DIST_ORDER, dist_counts()) for _ in range(c)]
    block, left = planted_block(seed, plan, pad=pad)
    assert not left, 'dist15: %d plants did not fit' % len(left)
    return block


def cyclic_text(counts):
    """{byte: count} as text in which no byte equals either of the two before it (so not even level 2's distances 1 and 2 match):
    round j holds, in order, every byte with a count above j.  At most 512 bytes, so that the hash table is still empty."""
    out = bytearray()
    for j in range(max(counts.values())):
        out += bytes(s for s in sorted(counts) if counts[s] > j)
    assert len(out) <= ROUND and sum(c == max(counts.values()) for c in counts.values()) >= 3
    return bytes(out)


def _crossing_run():
    # 128 planted matches whose distance counts 1 1 2 4 ... 64 give distances 1 and 2 seven bits each, and so many matches of 5 and 6
    # bytes (the last two length symbols in use) that these get seven bits too
    seed, n5, n6 = 1, 28, 22
    syms = [s for s, c in {0: 1, 1: 1, 18: 2, 19: 4, 20: 8, 21: 16, 22: 32, 23: 64}.items() for _ in range(c)]
    random.Random(seed).shuffle(syms)
    lens = [6] * n6 + [5] * n5 + [4] * (len(syms) - n5 - n6)
    random.Random(seed + 1).shuffle(lens)
    block, left = planted_block(seed, list(zip(syms, lens)), n=4000, pad=False)
    assert not left
    return block


# (seed, k, nfill, per, base), bytes
LIT15 = [((2, 21, 100, 2, 86), BLOCK), ((1, 21, 100, 3, 77), BLOCK), ((1, 22, 215, 1, 41), 61111), ((2, 21, 100, 2, 86), 60001)]
CLEN7 = [((2, 21, 150, 3, 221), BLOCK), ((1, 22, 150, 1, 157), BLOCK), ((2, 15, 215, 1, 130), BLOCK), ((1, 15, 100, 2, 166), BLOCK)]
LIMIT_OF = {'lit15': ('lit', 15), 'clen7': ('clen', 7), 'dist15': ('dist', 15)}


@functools.lru_cache(maxsize=None)
def limit_blocks():
    """[(name, block)]: the name's first part (lit15, clen7, dist15) is the limit the block reaches, at both levels."""
    out = []
    for kind, table in (('lit15', LIT15), ('clen7', CLEN7)):
        for (seed, k, nfill, per, base), n in table:
            b = filler_block(seed, k, nfill, per, base, n)
            out.append(('%s/s%d_k%d_f%d_p%d_b%d/%d' % (kind, seed, k, nfill, per, base, len(b)), b))
    for seed, pad in ((2, True), (4, False)):
        b = dist_block(seed, pad)
        out.append(('dist15/s%d/%d' % (seed, len(b)), b))
    return out


@functools.lru_cache(maxsize=None)
def header_blocks():
    """[(name, block)]: small blocks, each built for one shape of the dynamic header (test_deflate_limits_cpu.py says which)."""
    rnd = random.Random(20261019)
    out = [('hdr/empty', b''), ('hdr/one_byte', b'G')]
    out.append(('hdr/only_00_ff', b'\x00\xff' + bytes(rnd.choice(b'\x00\xff') for _ in range(1500))))
    text = bytearray()
    while len(text) < 400:
        v = rnd.choice(b'AAAACCCGGTTN\n')
        if v not in text[-2:]: text.append(v)
    out.append(('hdr/no_match', bytes(text)))
    w = bytes(rnd.randrange(64, 128) for _ in range(600))
    out.append(('hdr/one_distance_symbol', w + w))
    out.append(('hdr/run_crosses_hlit', _crossing_run()))
    out.append(('hdr/zero_runs_10_11', cyclic_text({0x20: 60, 0x2B: 60, 0x37: 60, 0x50: 30, 0x60: 10})))
    counts = {0x0A: 18}
    counts.update({s: 12 for s in range(0x30, 0x36)})       # 6, 8 and 7 neighbours with one length each
    counts.update({s: 18 for s in range(0x41, 0x49)})
    counts.update({s: 12 for s in range(0x61, 0x68)})
    out.append(('hdr/repeats_6_7_8', cyclic_text(counts)))
    return out


def fastq_blocks(k):
    """k whole blocks of ordinary FASTQ text"""
    from uq_amd import synth
    data = synth.fastq(20261019, 2000 * k, (36, 301), n_rate=1)
    assert len(data) >= k * BLOCK
    return [data[i * BLOCK:(i + 1) * BLOCK] for i in range(k)]
