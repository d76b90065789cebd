"""Hand-made FASTQ texts for the read trimmer's tests (tests/test_trim_cpu.py, tests/test_gpu_trim.py, tests/test_gpu_trim_cli.py)."""
import random

from filter_inputs import record, text

T = 20                                  # the quality threshold the shaped lines below are made for
HI, LO = b'I', b'#'                     # Phred 40 and 2: T - q = -20 and +18
LENGTHS = list(range(18)) + [63, 64, 65, 255, 256, 257]


def bases(L, seed=0):
    rnd = random.Random(seed * 7919 + L)
    return bytes(rnd.choice(b'ACT') for _ in range(L))        # no G, no N: only what a test puts at the ends is cut


def quality_cuts(lengths=LENGTHS, reach=17):
    """For every length L and every c <= min(L, reach): a read whose last c qualities are low (q3=T cuts exactly c: every position of the last
    two 8-byte chunks), and its mirror image for q5."""
    out = []
    for L in lengths:
        for c in range(min(L, reach) + 1):
            out.append(record(b'e%d_%d' % (L, c), bases(L, c), HI * (L - c) + LO * c))
            out.append(record(b's%d_%d' % (L, c), bases(L, c + 1), LO * c + HI * (L - c)))
    return text(out)


def quality_shapes(seed=1, n=120):
    """Running sums that are 0 all along (every quality equals T: the strict >), that stay close to 0 (qualities T - 1 .. T + 1), that go
    negative and later far positive (the stop must hold), and whose highest value and stop lie many chunks apart."""
    rnd = random.Random(seed)
    out = []
    for L in (1, 8, 9, 64, 150, 257):
        out.append(record(b'flat%d' % L, bases(L), bytes([33 + T]) * L))
    for k in range(n):
        L = rnd.randrange(1, 301)
        kind = k % 4
        if kind == 0: u = bytes(33 + T + rnd.choice((-1, 0, 0, 1)) for _ in range(L))
        elif kind == 1: u = bytes(33 + T + rnd.randrange(-6, 5) for _ in range(L))
        elif kind == 2:                  # ends: a little low, then good (the sum goes negative), then a long low stretch inside
            e = rnd.randrange(0, 9)
            mid = max(L - 2 * e - 8, 0)
            u = (LO * e + HI * 4 + LO * mid + HI * 4 + LO * e)[:L]
            u += HI * (L - len(u))
        else:                            # a high plateau: +18 for a while, -1 for long, then the stop
            up = rnd.randrange(1, 20)
            u = (HI * 3 + bytes([33 + T + 1]) * max(L - up - 6, 0) + LO * up)[:L]
            u = bytes(reversed(u)) if k % 8 == 3 else u
            u += HI * (L - len(u))
        out.append(record(b'q%d' % k, bases(L, k), u))
    return text(out)


def polyg_runs(G=10):
    """3' runs of G - 1, G and G + 1 G, the whole read, runs across an 8-byte and a 16-lane (128-byte) boundary, lower case, a run broken by one base."""
    out = []
    for r in (0, 1, G - 1, G, G + 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 200):
        for body in (0, 3, 60):
            out.append(record(b'g%d_%d' % (r, body), bases(body, r) + b'G' * r))
    out.append(record(b'lower', bases(20) + b'gGgGgGgGgGgG'))
    out.append(record(b'broken', bases(20) + b'GGGGGGGGAGGGGGGGGG'))
    out.append(record(b'broken_lc', bases(20) + b'GGGGGGGGGGGGGaGG'))
    out.append(record(b'allg', b'G' * 150))
    out.append(record(b'allg_lc', b'g' * 9))
    return text(out)


def n_ends():
    """N at both ends, in both cases, across 8-byte boundaries; reads that are all N; N inside only."""
    out = []
    for lead in (0, 1, 7, 8, 9, 17):
        for trail in (0, 1, 7, 8, 9, 40):
            out.append(record(b'n%d_%d' % (lead, trail), b'Nn' * (lead // 2) + b'N' * (lead % 2) + b'ACNGT' + b'n' * (trail % 2) + b'nN' * (trail // 2)))
    for L in (1, 7, 8, 9, 16, 17, 150):
        out.append(record(b'alln%d' % L, (b'Nn' * L)[:L]))
    out.append(record(b'inside', b'ACGTNNNNNNNNNNACGT'))
    return text(out)


def long_reads_among_short(seed=3):
    """Reads of 5000 bases (tiles beyond the stage) among short ones; their ends carry low qualities, G runs and N."""
    rnd = random.Random(seed)
    out = []
    for k in range(24):
        L = 5000 if k % 5 == 2 else rnd.randrange(20, 200)
        g, c, nn = rnd.randrange(0, 30), rnd.randrange(0, 40), rnd.randrange(0, 12)
        seq = (b'N' * nn + bases(L, k))[:L]
        seq = seq[:max(L - g, 0)] + b'G' * min(g, L)
        qual = bytes(33 + T + rnd.randrange(-3, 15) for _ in range(L))
        qual = (LO * nn + qual)[:max(L - c, 0)] + LO * min(c, L)
        out.append(record(b'm%d' % k, seq, qual))
    out.append(record(b'at4096', bases(4096), HI * 4000 + LO * 96))
    out.append(record(b'at4097', bases(4097), LO * 4097))
    return text(out)


def deep_record(L=70000):
    """A read of L bases whose quality cuts lie deep inside it and whose running sums stop in another step than the one that holds their
    highest value: from the 3' end 3000 low qualities (the sum climbs to 54 000), 10 000 of T + 1 (it sinks by one each), then Phred 93 (it
    goes negative some 600 bases on); behind the stop 20 000 low ones that must not count.  The 5' end is the same with 1700 / 9000."""
    t1 = bytes([33 + T + 1])
    five = LO * 1700 + t1 * 9000 + b'~' * 600
    three = b'~' * 1000 + t1 * 10000 + LO * 3000
    mid = L - len(five) - len(three)
    u = five + LO * 20000 + HI * (mid - 20000) + three
    assert len(u) == L
    return record(b'deep', bases(L), u)


def deep_text(where, others=12):
    small = [record(b's%d' % k, b'ACTGN' * (k % 4), None) for k in range(others)]
    at = {'first': 0, 'middle': others // 2, 'last': others}[where]
    return text(small[:at] + [deep_record()] + small[at:]), at


def hand_inputs():
    from filter_inputs import odd_quality_bytes, odd_shapes, edges_n
    yield 'quality cuts', quality_cuts(lengths=list(range(18)) + [63, 64, 65])
    yield 'quality shapes', quality_shapes()
    yield 'poly-G runs', polyg_runs()
    yield 'N ends', n_ends()
    yield 'odd quality bytes', odd_quality_bytes()
    yield 'odd shapes', odd_shapes()
    yield 'edges n', edges_n()


def mates(n=300, seed=41):
    """R1 and R2 of n pairs with Illumina names, reads of 36 .. 151 bases, one base in a hundred an N of low quality."""
    rnd = random.Random(seed)
    out = []
    for m in (1, 2):
        recs = []
        for i in range(n):
            L = rnd.randint(36, 151)
            seq = bytes(rnd.choice(b'ACGT') if rnd.random() > 0.01 else 78 for _ in range(L))
            recs.append(b'\n'.join((b'@A00:7:HX:%d:%d:%d %d:N:0:ACGT' % (1 + i % 4, 1000 + i // 7, 2000 + 3 * i, m), seq, b'+',
                                    bytes(35 if c == 78 else rnd.randint(36, 73) for c in seq))) + b'\n')
        out.append(b''.join(recs))
    return out


def interleave(a, b):
    ra, rb = a.split(b'\n')[:-1], b.split(b'\n')[:-1]
    return b''.join(b'\n'.join(ra[4 * i:4 * i + 4]) + b'\n' + b'\n'.join(rb[4 * i:4 * i + 4]) + b'\n' for i in range(len(ra) // 4))
