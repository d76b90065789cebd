"""Hand-made FASTQ texts for the read filter's tests (tests/test_filter_cpu.py, tests/test_gpu_filter.py)."""
import random


def record(name, seq, qual=None, plus=b'+'):
    if qual is None: qual = b'I' * len(seq)
    return b'@' + name + b'\n' + seq + b'\n' + plus + b'\n' + qual + b'\n'


def text(records):
    return b''.join(records)


def lengths(ls, seed=1, n_rate=0.0):
    """One record per length of `ls`: random bases (N at n_rate), random qualities '#'..'J'."""
    rnd = random.Random(seed)
    out = []
    for k, L in enumerate(ls):
        seq = bytes(rnd.choice(b'ACGT') if rnd.random() >= n_rate else rnd.choice(b'Nn') for _ in range(L))
        qual = bytes(rnd.randrange(35, 75) for _ in range(L))
        out.append(record(b'r%d' % k, seq, qual))
    return text(out)


def edges_len():
    """Sequence lengths 9, 10, 11 (around a threshold of 10), twice."""
    return lengths([9, 10, 11, 11, 10, 9], seed=2)


def edges_n():
    """N counts 2, 3, 4 around max_n = 3, in upper and lower case, at both ends of the line and in the 8-byte tail."""
    return text([record(b'a', b'NACGTACGTN'), record(b'b', b'NNACGTACGN'), record(b'c', b'NnACGTACnN'), record(b'd', b'nnnn'), record(b'e', b'nnn'),
                 record(b'f', b'ACGTACGTACGTACGTnnACGTAn'), record(b'g', b'ACGTACGTACGTACGTnnACGTnn'), record(b'h', b'')])


def edges_q():
    """SUM q against 20 * Lu: one below, at and above, on lines of 1, 7, 8, 9 and 40 qualities."""
    out = []
    for L in (1, 7, 8, 9, 40):
        for d in (-1, 0, 1):
            tot = 20 * L + d
            qs = [20] * L
            qs[-1] += d
            assert sum(qs) == tot
            out.append(record(b'q%d_%d' % (L, d + 1), b'A' * L, bytes(33 + v for v in qs)))
    return text(out)


def odd_quality_bytes():
    """Quality bytes outside 33 .. 126: they clamp to 0 and 93."""
    return text([record(b'lo', b'ACGT', bytes([0, 9, 32, 33])), record(b'hi', b'ACGT', bytes([126, 127, 200, 255])),
                 record(b'mix', b'ACGTACGTAC', bytes([255, 1, 255, 1, 255, 1, 255, 1, 255, 1])),
                 record(b'at', b'ACGTACGTA', bytes([34] * 8 + [11]))])


def odd_shapes():
    """Empty lines, Ls != Lu, CRLF line ends, text behind the +."""
    return text([record(b'', b'', b''), record(b'e1', b'', b'IIII'), record(b'e2', b'ACGT', b''), record(b'long_q', b'AC', b'IIIIIIIIII'),
                 record(b'long_s', b'ACGTNNNNAC', b'#'), b'@crlf\r\nACNT\r\n+\r\nIIII\r\n', record(b'p', b'ACGT', b'IIII', b'+p comment'),
                 b'\n\n\n\n', record(b'z', b'N', b'!')])


def hand_inputs():
    yield 'edges len', edges_len()
    yield 'edges n', edges_n()
    yield 'edges q', edges_q()
    yield 'odd quality bytes', odd_quality_bytes()
    yield 'odd shapes', odd_shapes()


def short_records(n=300, seed=3):
    rnd = random.Random(seed)
    return lengths([rnd.randrange(0, 40) for _ in range(n)], seed=seed, n_rate=0.05)


def tiny_records(n=41, seed=4):
    """Records of 4 to 14 bytes: the four newlines and up to ten other bytes, spread over the four lines."""
    rnd = random.Random(seed)
    out = []
    for k in range(n):
        extra = rnd.randrange(0, 11)
        cut = sorted(rnd.randrange(0, extra + 1) for _ in range(3))
        parts = [cut[0], cut[1] - cut[0], cut[2] - cut[1], extra - cut[2]]
        out.append(b''.join(bytes(rnd.choice(b'ACGTN#I@+') for _ in range(p)) + b'\n' for p in parts))
    return text(out)


def sized_record(size, fill=b'ACGT'):
    """A record of exactly `size` bytes, size >= 7."""
    name = b'x' if size % 2 else b''
    L = (size - 6 - len(name)) // 2
    seq = (fill * (L // len(fill) + 1))[:L]
    r = record(name, seq, bytes(40 + (k * 7) % 50 for k in range(L)))
    assert len(r) == size
    return r


def numbered_records(n):
    """n short records whose content says which they are (cheap to make: the sampled compaction takes 20 000)."""
    return text([record(b'%d' % k, b'ACGTN'[:k % 5] * (k % 7), None) for k in range(n)])


def four_byte_units(n):
    return b'\n\n\n\n' * n


def long_record_text(where, L=70000, others=12, seed=5):
    """A read of L bases among `others` short ones: first, in the middle or last."""
    rnd = random.Random(seed)
    seq = bytes(rnd.choice(b'ACGTN') for _ in range(L))
    qual = bytes(rnd.randrange(33, 80) for _ in range(L))
    big = record(b'big', seq, qual)
    small = [record(b's%d' % k, b'ACGTN' * (k % 4), None) for k in range(others)]
    at = {'first': 0, 'middle': others // 2, 'last': others}[where]
    return text(small[:at] + [big] + small[at:]), at


def pairs_text(n=60, seed=6):
    """An interleaved text: pair i's mates have different lengths and N counts."""
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        for m in (1, 2):
            L = rnd.randrange(5, 60)
            seq = bytes(rnd.choice(b'ACGT') if rnd.random() > 0.08 else 78 for _ in range(L))
            out.append(record(b'p%d/%d' % (i, m), seq, bytes(rnd.randrange(35, 74) for _ in range(L))))
    return text(out)
