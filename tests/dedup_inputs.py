"""Hand-made FASTQ texts for the duplicate remover's tests (tests/test_dedup_cpu.py, tests/test_gpu_dedup.py): deterministic, small, one
property each."""
import random

EDGE_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65)      # the hash word and the 16-byte vector edges
TILE_RECORDS = 64                                            # the keys kernel's largest tile (DK_RMAX in dedup.hip)
STAGE = 20480                                                # its staging bytes (DK_CAP)


def record(i, s, u=None):
    s = bytes(s)
    return b'@r%d\n' % i + s + b'\n+\n' + (bytes(u) if u is not None else b'I' * len(s)) + b'\n'


def text_of(seqs, quals=None):
    return b''.join(record(i, s, quals[i] if quals else None) for i, s in enumerate(seqs))


def rand_seq(rng, n, letters=b'ACGT'):
    return bytes(rng.choice(letters) for _ in range(n))


def edge_lengths():
    """Every edge length three times: a copy right behind, a copy far behind, and a text that differs in its last byte."""
    rng = random.Random(1)
    seqs = [rand_seq(rng, n) for n in EDGE_LENGTHS]
    near = [s[:-1] + (b'A' if s[-1:] != b'A' else b'C') for s in seqs if s]
    out = []
    for s in seqs: out += [s, s]
    return text_of(out + near + seqs)


def near_misses():
    """Texts that differ only in the last byte, only in length (the longer one's extra byte has zero low bits or is all zero, so the padded
    hash words are close or equal), only in case; N equals N."""
    seqs = [b'ACG', b'ACGA', b'ACG@', b'ACG\x00', b'ACG', b'acg', b'ACg', b'ACGA', b'ACGT', b'ACGN', b'ACGN', b'ACGn',
            b'ACGTACGT', b'ACGTACGT\x00', b'ACGTACGT', b'ACGTACGA', b'', b'', b'\x00', b'\x00\x00', b'\x00']
    return text_of(seqs)


def counted(units, unit=1, seed=2):
    """`units` units of reads of 20 .. 90 bases, every fifth a copy of an earlier one."""
    rng = random.Random(seed * 1000 + units)
    seqs = []
    for w in range(units):
        if w % 5 == 4: seqs += seqs[unit * rng.randrange(w):][:unit]
        else: seqs += [rand_seq(rng, rng.randrange(20, 91)) for _ in range(unit)]
    return text_of(seqs)


def spread(n=20000, dup=0.10, seed=3, lo=36, hi=152):
    """n reads, about `dup` of them copies: of the read right in front (the same tile), of one a tile back (the neighbouring tile), and of a
    read anywhere before (far-apart workgroups), in equal parts.  Qualities vary, so keep=best has something to choose."""
    rng = random.Random(seed)
    seqs, quals = [], []
    for i in range(n):
        if i > TILE_RECORDS and rng.random() < dup:
            j = (i - 1, i - TILE_RECORDS, rng.randrange(i))[rng.randrange(3)]
            s = seqs[j]
        else:
            s = rand_seq(rng, rng.randrange(lo, hi), b'ACGTACGTACGTN')
        seqs.append(s)
        quals.append(bytes(rng.choice(b'#5?DI') for _ in range(len(s))))
    return text_of(seqs, quals)


def one_class(copies=1000):
    """One class of `copies` copies among other reads."""
    rng = random.Random(4)
    s = rand_seq(rng, 100)
    seqs = [rand_seq(rng, 100) if i % 3 == 1 else s for i in range(copies * 3 // 2)]
    return text_of(seqs)


def pairs():
    """Interleaved pairs: copies of whole pairs, pairs where only mate 2 differs, pairs with the mates swapped."""
    rng = random.Random(5)
    a, b, c, d = (rand_seq(rng, n) for n in (50, 60, 50, 60))
    seqs = [a, b, a, b, a, d, b, a, c, b, a, b, b, a, a, a, a, a, b'', b'', b'', a, b'', b'']
    return text_of(seqs)


def long_run():
    """Short reads with a run of long ones in the middle: the run's tiles pass the stage and are read straight from HBM; copies inside the
    run, and of the run's reads among the short ones."""
    rng = random.Random(6)
    short = [rand_seq(rng, 50) for _ in range(1500)]
    run = [rand_seq(rng, 600) for _ in range(40)]
    run = run + run[:20] + [r[:-1] + b'A' for r in run[20:30]]
    seqs = short[:700] + run + short[700:] + run[5:9] + short[10:14]
    return text_of(seqs)


def huge_line(copies):
    """One line of 70 000 bases (beyond the whole-workgroup threshold), `copies` times, among short reads."""
    rng = random.Random(7)
    big = rand_seq(rng, 70000)
    seqs = [rand_seq(rng, 80) for _ in range(6)]
    for k in range(copies): seqs.insert(2 + 3 * k, big)
    seqs.append(big[:-1] + b'N')                                # the same but for its last byte
    return text_of(seqs)


def score_ties():
    """Equal texts with chosen quality sums: ties go to the lower index, a higher sum later wins."""
    s = b'ACGTACGTAC'
    quals = [b'5555555555', b'IIIIIIIIII', b'IIIIIIIIII', b'5555555555', b'IIIIIIIII5', b'5IIIIIIIII', b'~~~~~~~~~~', b'\x7f\x7f\x7f\x7f\x7f\x7f\x7f\x7f\x7f\xff',
             b'!!!!!!!!!!', b'\x00\x01\x02\x03\x04\x05\x06\x07\x08\x09']
    return text_of([s] * len(quals) + [b'TTTT', b'TTTT'], quals + [b'!!!!', b'!!!!'])


def score_clamp():
    """Three equal reads whose quality sums are 2^32 - 2, 2^32 - 1 and beyond 2^32: the last two tie at the clamp, the lower index wins."""
    full, rest = divmod((1 << 32) - 2, 93)
    base = b'~' * full + bytes([33 + rest])
    return text_of([b'ACGT'] * 3, [base, base + b'"', base + b'~' * 3])


def hand_inputs():
    yield 'edge_lengths', edge_lengths()
    yield 'near_misses', near_misses()
    yield 'pairs', pairs()
    yield 'score_ties', score_ties()
    yield 'one_class', one_class(60)
    for units in (1, 2, 63, 64, 65, 129):
        yield 'counted_%d' % units, counted(units)
