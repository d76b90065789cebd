"""Paired-end input (include/uqhip.h) in plain Python, written from the definitions and independent of the library:
the interleave of two FASTQ texts record by record, and the mate rule on two QNAME lines."""

UINT64_MAX = (1 << 64) - 1


def records(text):
    """The records of a FASTQ text, each with its four newlines."""
    lines = text.split(b'\n')
    assert lines[-1] == b'' and (len(lines) - 1) % 4 == 0, 'not whole FASTQ records'
    return [b''.join(l + b'\n' for l in lines[4 * r:4 * r + 4]) for r in range((len(lines) - 1) // 4)]


def interleave(a, b, first_pair=0, npairs=None):
    """A(first) B(first) A(first + 1) B(first + 1) ..."""
    ra, rb = records(a), records(b)
    if npairs is None:
        assert len(ra) == len(rb)
        npairs = len(ra) - first_pair
    return b''.join(ra[r] + rb[r] for r in range(first_pair, first_pair + npairs))


def qname(record):
    return record[:record.index(b'\n')]


def mate_id(line):
    """The bytes of a QNAME line (without its newline) in front of its first space or tab."""
    for k, c in enumerate(line):
        if c in b' \t': return line[:k]
    return line


def mates(line_a, line_b):
    """(the pair matches, its /1 and /2 were dropped)"""
    ia, ib = mate_id(line_a), mate_id(line_b)
    slash = ia.endswith(b'/1') and ib.endswith(b'/2')
    if slash: ia, ib = ia[:-2], ib[:-2]
    return ia == ib, slash


def report(names_a, names_b, pair_index_base=0, into=None):
    """The uq_mate_report of these pairs of QNAME lines, as a dict; `into`: an earlier report to add to."""
    r = dict(into) if into else {'pairs': 0, 'mismatches': 0, 'first_mismatch': None, 'slash_pairs': 0}
    assert len(names_a) == len(names_b)
    for i, (x, y) in enumerate(zip(names_a, names_b)):
        ok, slash = mates(x, y)
        r['pairs'] += 1
        r['slash_pairs'] += slash
        if not ok:
            r['mismatches'] += 1
            if r['first_mismatch'] is None or pair_index_base + i < r['first_mismatch']: r['first_mismatch'] = pair_index_base + i
    return r


def check_texts(a, b, first_a=0, step_a=1, first_b=0, step_b=1, npairs=None, pair_index_base=0, into=None):
    """The report of pair i = (record first_a + i step_a of a, record first_b + i step_b of b)."""
    ra, rb = records(a), records(b)
    if npairs is None: npairs = min(len(range(first_a, len(ra), step_a)), len(range(first_b, len(rb), step_b)))
    return report([qname(ra[first_a + i * step_a]) for i in range(npairs)], [qname(rb[first_b + i * step_b]) for i in range(npairs)], pair_index_base, into)
