"""Hand-made inputs of the paired-end tests (tests/test_pairs_cpu.py holds the host twins to them, tests/test_gpu_pairs.py the kernels):
FASTQ texts whose records put segment boundaries where the interleave kernel can go wrong, and pairs of QNAME lines for the mate rule."""
import random


def text_of(records):
    return b''.join(b'\n'.join(r) + b'\n' for r in records)


def line(rnd, L, alphabet):
    return bytes(rnd.choice(alphabet) for _ in range(L))


QUALS = bytes(range(33, 127))


def read(rnd, name, L):
    return (name, line(rnd, L, b'ACGTN'), b'+', line(rnd, L, QUALS))


def record_bytes(name, L):
    return len(name) + 2 * L + 5


def one_pair():
    rnd = random.Random(1)
    return text_of([read(rnd, b'@only', 21)]), text_of([read(rnd, b'@only', 34)])


def tiny_pairs(n=40, seed=2):
    """Records of 7 to 14 bytes (a '@' and 1 to 3 characters, 0 to 2 bases, every size from 9 to 14 among them): an output vector holds
    up to three segments."""
    rnd = random.Random(seed)
    a, b = [], []
    for i in range(n):
        name = b'@' + bytes(rnd.choice(b'abcxyz') for _ in range(1 + i % 3))
        a.append(read(rnd, name, (i // 3) % 3))
        b.append(read(rnd, name, (i // 2 + 1) % 3))
    sizes = {record_bytes(r[0], len(r[1])) for r in a + b}
    assert set(range(9, 14)) <= sizes and min(sizes) >= 7
    a.append(read(rnd, b'@abcd', 2)); b.append(read(rnd, b'@abcd', 2))      # 14 bytes
    return text_of(a), text_of(b)


def unequal_pairs(n=60, seed=3):
    """151 bp with 36 bp, then lengths 1 to 300 on both sides."""
    rnd = random.Random(seed)
    a = [read(rnd, b'@m%d/1' % i, 151) for i in range(n)] + [read(rnd, b'@v%d' % i, rnd.randint(1, 300)) for i in range(n)]
    b = [read(rnd, b'@m%d/2' % i, 36) for i in range(n)] + [read(rnd, b'@v%d' % i, rnd.randint(1, 300)) for i in range(n)]
    return text_of(a), text_of(b)


def edge_pairs(tile, d, which, phase=0, seed=4):
    """Pairs whose segment boundary number `which` (1: the end of A(0), 2: the end of B(0), 3: the end of A(1)) falls d bytes behind the
    edge of the output's first tile, for an output buffer that begins `phase` bytes past a 16-byte boundary: the tile ends at output
    offset tile - phase.  Short pairs follow."""
    rnd = random.Random(seed * 1000 + d * 8 + which)
    want = tile - phase + d                                          # output offset of the boundary
    # A(0) = '@e' + L0 bases; B(0) = '@e' + 3 bases (11 bytes); A(1) = '@f' + 1 base (9 bytes)
    fixed = {1: 0, 2: record_bytes(b'@e', 3), 3: record_bytes(b'@e', 3) + record_bytes(b'@f', 1)}[which]
    rest = want - fixed                                              # = the bytes of A(0) = 7 + 2 L0 or, with a three-byte name, 8 + 2 L0
    name0 = b'@e' if (rest - 7) % 2 == 0 else b'@ee'
    L0 = (rest - record_bytes(name0, 0)) // 2
    assert L0 >= 0 and record_bytes(name0, L0) == rest
    a = [read(rnd, name0, L0), read(rnd, b'@f', 1)] + [read(rnd, b'@s%d' % i, i % 7) for i in range(30)]
    b = [read(rnd, b'@e', 3), read(rnd, b'@f', 2)] + [read(rnd, b'@s%d' % i, (i + 3) % 5) for i in range(30)]
    a, b = text_of(a), text_of(b)
    return a, b, want


def many_pairs_in_a_tile(n=700, seed=5):
    """Pairs of some 20 bytes: more than 256 of them inside one 16 KiB tile."""
    rnd = random.Random(seed)
    a = [read(rnd, b'@%d' % (i % 10), i % 3) for i in range(n)]
    b = [read(rnd, b'@%d' % (i % 10), (i + 1) % 3) for i in range(n)]
    return text_of(a), text_of(b)


def long_record_pairs(where, seed=6):
    """A 70 000-base record (longer than a tile) among short ones: `where` = 'first', 'middle' or 'last', in a or in b."""
    rnd = random.Random(seed)
    n = 41
    at = {'first': 0, 'middle': n // 2, 'last': n - 1}[where]
    a = [read(rnd, b'@r%d' % i, 70000 if i == at else 5 + i % 40) for i in range(n)]
    b = [read(rnd, b'@r%d' % i, 70000 if i == (at + 1) % n else 3 + i % 30) for i in range(n)]
    return text_of(a), text_of(b)


def name_pair(x, y):
    """Two one-record texts with these QNAME lines."""
    return text_of([(x, b'AC', b'+', b'II')]), text_of([(y, b'ACG', b'+', b'III')])


LONG = b'@' + bytes(97 + i % 26 for i in range(299))
# (QNAME of a, QNAME of b, the pair matches, its /1 and /2 are dropped)
RULE_CASES = [
    (b'@read7', b'@read7', True, False),
    (b'@read7/1', b'@read7/2', True, True),
    (b'@read7/2', b'@read7/1', False, False),
    (b'@read7/1', b'@read7/1', True, False),
    (b'@read7/2', b'@read7/2', True, False),
    (b'@x/1', b'@y/2', False, True),                                # dropped, and still no match
    (b'@A00 1:N:0:ACGT', b'@A00 2:N:0:ACGT', True, False),
    (b'@A00\t1:N:0:ACGT', b'@A00\t2:N:0:ACGT', True, False),
    (b'@A00/1 1:N:0:ACGT', b'@A00/2\t2:N:0:ACGT', True, True),
    (b'@A00 1:N:0:ACGT', b'@A01 1:N:0:ACGT', False, False),
    (b'@r1', b'@r10', False, False),
    (b'@r10', b'@r1', False, False),
    (b'@r1', b'@r1 0', True, False),
    (b'@', b'@', True, False),
    (b'@', b'@a', False, False),
    (b'@ a', b'@ b', True, False),
    (b'', b'', True, False),
    (b'/1', b'/2', True, True),
    (b'@abcdefg', b'@abcdefg', True, False),                        # 8 bytes: one whole word
    (b'@abcdefgh', b'@abcdefgX', False, False),
    (b'@abcdef/1', b'@abcdef/2', True, True),                       # the dropped bytes begin a second word
    (b'@abcde/1', b'@abcde/2', True, True),
    (LONG, LONG, True, False),
    (LONG, LONG[:-1] + b'!', False, False),
    (LONG, b'#' + LONG[1:], False, False),
    (LONG + b'/1', LONG + b'/2', True, True),
    (LONG + b' x', LONG + b'\ty', True, False),
]


def names_text(names, seed=7, lo=1, hi=40):
    rnd = random.Random(seed)
    return text_of([read(rnd, nm, rnd.randint(lo, hi)) for nm in names])


def mismatch_texts(n, bad):
    """n pairs of equal names, those at the positions `bad` renamed in b."""
    na = [b'@q%d' % i for i in range(n)]
    nb = [b'@Q%d' % i if i in bad else b'@q%d' % i for i in range(n)]
    return names_text(na, 8), names_text(nb, 9)


def random_pairs(n=1000, rate=0.05, seed=10):
    rnd = random.Random(seed)
    na, nb = [], []
    for i in range(n):
        stem = b'@M0:%d:%d' % (rnd.randrange(10 ** rnd.randint(1, 9)), i)
        style = rnd.randrange(4)
        x, y = {0: (stem, stem), 1: (stem + b'/1', stem + b'/2'), 2: (stem + b' 1:N:0:AC', stem + b' 2:N:0:AC'),
                3: (stem + b'/1\tc', stem + b'/2\tc')}[style]
        if rnd.random() < rate:
            kind = rnd.randrange(4)
            yb = bytearray(y)
            if kind == 0: yb[rnd.randrange(1, len(stem))] ^= 1
            elif kind == 1: yb = bytearray(y[:len(stem) - 1] + y[len(stem):])
            elif kind == 2: yb = bytearray(b'@' + y)
            else: x, yb = y, bytearray(x)                           # swapped mates: /2 with /1
            y = bytes(yb)
        na.append(x); nb.append(y)
    return names_text(na, seed + 1), names_text(nb, seed + 2)
