"""FASTQ files built byte by byte for the exact tests of the statistics pass (tests/test_gpu_stats_exact.py, tests/test_oracle_c.py).
TEST INFRASTRUCTURE ONLY.  A record is (name, seq, qual) or (name, seq, qual, third line); no byte of a line may be 10."""
import numpy as np

NONE = (1 << 64) - 1


def fastq(records):
    out = []
    for rec in records:
        name, seq, qual = rec[:3]
        plus = rec[3] if len(rec) > 3 else b'+'
        for line in (name, seq, qual, plus):
            assert 10 not in line
        out.append(name + b'\n' + seq + b'\n' + plus + b'\n' + qual + b'\n')
    return np.frombuffer(b''.join(out), dtype=np.uint8).copy()


def first_appearance(records, first=0, count=None):
    """The base bytes of records [first, first + count) in the order a scan of the lines meets them (what the reference's dict keeps)."""
    seen = []
    for rec in records[first:len(records) if count is None else first + count]:
        seq = rec[1][:min(len(rec[1]), len(rec[2]))]                     # pairs are counted up to the shorter of SEQ and QUAL
        fresh = [b for b in set(seq) if b not in seen]
        seen += sorted(fresh, key=lambda b: seq.index(bytes([b])))
    return seen


def order_of_keys(keys):
    """(the bases sorted by their first-occurrence key, the set of bases without one) of a uq_first_occurrence / uqo_stats table."""
    keys = np.asarray(keys, dtype=np.uint64)
    present = [b for b in range(256) if int(keys[b]) != NONE]
    assert len({int(keys[b]) for b in present}) == len(present)          # two bases never share a (read, position)
    return sorted(present, key=lambda b: int(keys[b])), set(range(256)) - set(present)


LONG_READ = (1 << 20) + 64


def long_read_records():
    """Read 0 has 2^20 + 64 bases: 'A' everywhere except 'X' at position 6 (and again later) and 'Y' first at position 2^20 + 5.  X and
    Y carry one quality each ('I'), which A carries too (next to 'J'): both are N-trick candidates whose quality is shared, so their
    N_qual codes are numbered in the order the reference's dict met them -- X, then Y.  A key that keeps only 20 bits of the position
    sees Y at position 5, in front of X.  Two ordinary reads follow (their names give pass 1 a separator to infer)."""
    seq = bytearray(b'A' * LONG_READ)
    qual = bytearray(b'I' * LONG_READ)
    for p in range(0, LONG_READ, 2): qual[p + 1] = ord('J')
    for p in (6, 1000, (1 << 20) + 6): seq[p] = ord('X'); qual[p] = ord('I')
    for p in ((1 << 20) + 5, (1 << 20) + 40): seq[p] = ord('Y'); qual[p] = ord('I')
    return [(b'@q.1.a', bytes(seq), bytes(qual)), (b'@q.2.b', b'ACGTACGT', b'IIIIJJJJ'), (b'@q.3.c', b'TTGCA', b'JIJIJ')]
