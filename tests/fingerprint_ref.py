"""The FASTQ record fingerprint `uqfp1` in plain Python, from its definition alone; nothing of uq_amd is used.

All arithmetic is mod 2^64.  K = 0x9E3779B97F4A7C15; mix() is the splitmix64 finaliser without the increment.  A line b[0, L) (no newline)
is cut into little-endian u64 words w_k of b[8k, 8k + 8), zero-padded;  acc = sum_k mix(w_k + K (k + 1));  LH(tag, b) = mix(acc + K L + tag).
Record r (global, 0-based) with lines q, s, p, u:  hq = LH(1, q), hs = LH(2, s), hu = LH(4, u), pair = mix(hs + mix(hu)), rec = mix(hq + pair),
ord = mix(rec + K (r + 1)).  The fingerprint: reads, bases = sum len(s), plus_text = records whose line 3 is not exactly '+', and the sums of
hq, hs, hu, pair, rec, ord."""
M = (1 << 64) - 1
K = 0x9E3779B97F4A7C15
FIELDS = ('reads', 'bases', 'plus_text', 'qname', 'dna', 'qual', 'pairs', 'records', 'ordered')


def mix(x):
    x &= M
    x ^= x >> 30; x = x * 0xBF58476D1CE4E5B9 & M
    x ^= x >> 27; x = x * 0x94D049BB133111EB & M
    return x ^ (x >> 31)


def line_hash(tag, b):
    acc = 0
    for k in range((len(b) + 7) // 8):
        acc += mix(int.from_bytes(b[8 * k:8 * k + 8], 'little') + K * (k + 1))
    return mix(acc + K * len(b) + tag)


def record_hashes(q, s, u, r):
    hq, hs, hu = line_hash(1, q), line_hash(2, s), line_hash(4, u)
    pair = mix(hs + mix(hu))
    rec = mix(hq + pair)
    return hq, hs, hu, pair, rec, mix(rec + K * (r + 1))


def fingerprint_records(records, read_index_base=0):
    """records: (q, s, p, u) byte strings without newlines."""
    fp = dict.fromkeys(FIELDS, 0)
    for i, (q, s, p, u) in enumerate(records):
        fp['reads'] += 1; fp['bases'] += len(s); fp['plus_text'] += p != b'+'
        for name, h in zip(FIELDS[3:], record_hashes(q, s, u, read_index_base + i)):
            fp[name] = (fp[name] + h) & M
    return fp


def records_of(text):
    """The records of a FASTQ text whose every line ends in a newline."""
    lines = bytes(text).split(b'\n')
    assert lines[-1] == b'' and (len(lines) - 1) % 4 == 0, 'not whole records'
    return list(zip(*[iter(lines[:-1])] * 4))


def fingerprint(text, first_read=0, nreads=None, read_index_base=0):
    recs = records_of(text)
    recs = recs[first_read:] if nreads is None else recs[first_read:first_read + nreads]
    return fingerprint_records(recs, read_index_base)


def add(a, b):
    """Shards add."""
    return {k: (a[k] + b[k]) & M for k in FIELDS}
