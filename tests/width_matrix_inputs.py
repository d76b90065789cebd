"""Inputs for the symbol-width matrix (test_width_matrix_cpu.py, test_gpu_width_matrix.py): FASTQ text whose base and quality
alphabets have a chosen width of 1 .. 8 bits each, with the encoding parameters that go with it.  Plain Python and numpy, no
product code: the parameters are made here and not by decide(), which never yields width 1 and cannot be steered to most widths.

case(bd, bq, variable, ntrick, alphabet) -> dict
    fastq       the text (bytes), n records named @r:<i>:<i mod 3> (@r:<i> alone leaves the QNAME analysis no separator: the
                reference refuses such names, Q13, and so does the product)
    bases, qualities, N_qual, bits_per_base, bits_per_quality, variable_read_lengths, dna_max,
    Cd = dna_bytes_per_row, Cq = quality_bytes_per_row, n
    lengths     the read lengths
    carry       the N code does not fit bq bits (Q9 with a carry: the exact big-integer packer runs)
    decodable   every N code is a code of the quality alphabet (the rule of the existing tests: a NEW code, Q9, is not
                decodable by the reference either)

ladder_case(bd, bq, dna_max, n, short=None) -> the same dict for few, long reads (vectorised): fixed length dna_max, or -- with
`short` -- reads of 1 .. short characters and one of dna_max in the middle.
"""
import functools

import numpy as np

# symbols per width: inside the width's range (2^(b-1) < count <= 2^b; width 1 = two symbols) and, from three bits on, short of its end, so that the width is no
# accident of rounding
SYMBOLS = {1: 2, 2: 4, 3: 7, 4: 13, 5: 29, 6: 61, 7: 100, 8: 150}
FIXED_LENGTHS = (1, 3, 8, 13, 67)
# a partial group alone, full groups alone, both; b * L mod 8 takes every residue the width allows; 67 lies beyond the 66-character
# chunk switch of the tile decoder
VARIABLE_LENGTHS = (1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 33, 64, 67)
N_READS = 120
NTRICKS = (None, 'shared', 'new')
ALPHABETS = ('letters', 'scattered')
N_RATE = 0.10

_UPPER = 'ABCDEFGHIJKLMOPQRSTUVWXYZ'                    # (no N: the N-trick's base is never one of the alphabet)
_LOWER = 'abcdefghijklmnopqrstuvwxyz'
_DIGITS = '0123456789'


def width_of(count):
    """The width b with 2^(b-1) < count <= 2^b; two symbols and fewer: 1."""
    b = 1
    while (1 << b) < count: b += 1
    return b


def _letters_bases(count):
    if count == 2: return 'AC'
    if count == 4: return 'ACGT'
    if count == 7: return 'ACGHMRT'                      # low three bits of the characters all differ: the packer's 3-bit lookup-free form
    pool = 'ACGTRYKMSWBDHV'                              # IUPAC first, then the other letters, digits, then other bytes
    pool += ''.join(c for c in _UPPER + _LOWER + _DIGITS if c not in pool)
    pool += ''.join(chr(c) for c in range(33, 256) if chr(c) not in pool and c != ord('N'))
    return ''.join(sorted(pool[:count]))


def _letters_qualities(count):
    return ''.join(chr(33 + i) for i in range(count))   # one contiguous run from '!' (beyond 127 from 96 symbols on)


def _scattered(count, seed, exclude):
    """`count` of the bytes 1 .. 255 without newline, carriage return and `exclude`, seeded, sorted, never one contiguous run."""
    pool = np.array([c for c in range(1, 256) if c not in (10, 13) and c not in exclude])
    rng = np.random.default_rng(seed)
    while True:
        pick = np.sort(rng.choice(pool, count, replace=False))
        if int(pick[-1]) - int(pick[0]) + 1 != count: break
    return ''.join(chr(int(c)) for c in pick)


def alphabets(bd, bq, alphabet):
    """(bases, qualities) of SYMBOLS[bd] and SYMBOLS[bq] characters, sorted as the reference sorts them."""
    if alphabet == 'letters':
        return _letters_bases(SYMBOLS[bd]), _letters_qualities(SYMBOLS[bq])
    assert alphabet == 'scattered'
    return _scattered(SYMBOLS[bd], 1000 + bd, {ord('N')}), _scattered(SYMBOLS[bq], 2000 + bq, set())


def _row_bytes(bits, dna_max, variable):
    return -(-bits * (dna_max + (1 if variable else 0)) // 8)


def _symbols(rng, lengths, bases, qualities, ntrick):
    """Flat base and quality bytes for reads of the given lengths.  Every symbol of both alphabets comes once at the front
    (as far as the text reaches), the rest is drawn; with an N-trick a tenth of the positions is N with its one quality."""
    total = int(np.sum(lengths))
    B = np.frombuffer(bases.encode('latin-1'), np.uint8)
    Q = np.frombuffer(qualities.encode('latin-1'), np.uint8)
    Qfree = Q[:-1] if ntrick == 'shared' else Q          # 'shared': the last quality is N's alone
    s = rng.choice(B, total); q = rng.choice(Qfree, total)
    kb, kq = min(total, len(B)), min(total, len(Qfree))
    s[:kb] = rng.permutation(B)[:kb]; q[:kq] = rng.permutation(Qfree)[:kq]
    N_qual = {}
    if ntrick is not None:
        at = rng.random(total) < N_RATE
        if not at.any(): at[int(rng.integers(0, total))] = True
        s[at] = ord('N')
        if ntrick == 'shared':
            q[at] = Q[-1]; N_qual = {'N': len(qualities) - 1}
        else:
            q[at] = Q[0]; N_qual = {'N': len(qualities) + 1}      # the reference's Q9 rule: a NEW code, one beyond the next free one
    return s, q, N_qual


def _text(lengths, s, q, name=lambda i: b'@r:%d:%d' % (i, i % 3)):
    recs = []
    pos = 0
    for i, L in enumerate(lengths):
        L = int(L)
        recs.append(name(i) + b'\n' + s[pos:pos + L].tobytes() + b'\n+\n' + q[pos:pos + L].tobytes() + b'\n')
        pos += L
    return b''.join(recs)


def _case(bd, bq, variable, ntrick, bases, qualities, lengths, dna_max, seed, **kw):
    rng = np.random.default_rng(seed)
    s, q, N_qual = _symbols(rng, lengths, bases, qualities, ntrick)
    carry = bool(N_qual) and max(N_qual.values()) >= 2 ** bq
    Cd, Cq = _row_bytes(bd, dna_max, variable), _row_bytes(bq, dna_max, variable)
    return dict(fastq=_text(lengths, s, q, **kw), bases=bases, qualities=qualities, N_qual=N_qual, bits_per_base=bd, bits_per_quality=bq,
                variable_read_lengths=bool(variable), dna_max=int(dna_max), n=len(lengths), lengths=[int(L) for L in lengths],
                Cd=Cd, Cq=Cq, dna_bytes_per_row=Cd, quality_bytes_per_row=Cq,
                carry=carry, decodable=all(v < len(qualities) for v in N_qual.values()))


@functools.lru_cache(maxsize=None)
def case(bd, bq, variable, ntrick, alphabet):
    assert 1 <= bd <= 8 and 1 <= bq <= 8 and ntrick in NTRICKS and alphabet in ALPHABETS
    bases, qualities = alphabets(bd, bq, alphabet)
    k = NTRICKS.index(ntrick) * len(ALPHABETS) + ALPHABETS.index(alphabet)
    if variable:
        dna_max = max(VARIABLE_LENGTHS)
        lengths = [VARIABLE_LENGTHS[(i + k) % len(VARIABLE_LENGTHS)] for i in range(N_READS)]
    else:
        dna_max = FIXED_LENGTHS[(bd + bq + k) % len(FIXED_LENGTHS)]          # in turn: the six fixed cases of a width pair take all five
        lengths = [dna_max] * N_READS
    seed = ((bd * 8 + bq) * 2 + bool(variable)) * 6 + k
    return _case(bd, bq, variable, ntrick, bases, qualities, lengths, dna_max, 77_000 + seed)


def all_cases():
    """The parameters of the full product, in a fixed order."""
    return [(bd, bq, variable, ntrick, alphabet) for bd in range(1, 9) for bq in range(1, 9) for variable in (False, True)
            for ntrick in NTRICKS for alphabet in ALPHABETS]


def case_id(bd, bq, variable, ntrick, alphabet):
    return '%d.%d-%s-%s-%s' % (bd, bq, 'variable' if variable else 'fixed', ntrick or 'plain', alphabet)


@functools.lru_cache(maxsize=None)
def ladder_case(bd, bq, dna_max, n, short=None):
    """Few, long reads with scattered alphabets and the shared N-trick: n reads of dna_max characters, or (short given) reads of
    1 .. short characters with one of dna_max characters in the middle."""
    bases, qualities = alphabets(bd, bq, 'scattered')
    rng = np.random.default_rng(88_000 + (bd * 8 + bq) * 131 + dna_max % 9973 + n)
    if short is None:
        lengths = [dna_max] * n
    else:
        lengths = [int(L) for L in rng.integers(1, short + 1, n)]
        lengths[n // 2] = dna_max
    return _case(bd, bq, short is not None, 'shared', bases, qualities, lengths, dna_max, 99_000 + bd * 8 + bq + dna_max)


def printable_case(bd, bq, variable, nb=None, nq=None):
    """A case for the command line: scattered printable ASCII, no N-trick (every base meets several qualities), alphabets of
    nb / nq symbols (default: SYMBOLS, cut to what printable ASCII holds), names of a family the reference's QNAME analysis accepts."""
    pool = np.arange(33, 127)
    nb = nb or min(SYMBOLS[bd], 70); nq = nq or min(SYMBOLS[bq], 70)
    rng = np.random.default_rng(55_000 + bd * 8 + bq)

    def pick(count):
        while True:
            p = np.sort(rng.choice(pool, count, replace=False))
            if int(p[-1]) - int(p[0]) + 1 != count: return ''.join(chr(int(c)) for c in p)
    bases, qualities = pick(nb), pick(nq)
    if variable:
        dna_max = max(VARIABLE_LENGTHS)
        lengths = [VARIABLE_LENGTHS[i % len(VARIABLE_LENGTHS)] for i in range(N_READS)]
    else:
        dna_max = 13
        lengths = [dna_max] * N_READS
    return _case(bd, bq, variable, None, bases, qualities, lengths, dna_max, 66_000 + bd * 8 + bq, name=lambda i: b'@q:%d:%d' % (i % 7, 3 * i + 1))
