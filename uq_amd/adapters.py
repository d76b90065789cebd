"""--adapter SPEC: which 3' adapter an encode finds and cuts off its reads (an extension; DESIGN.md section 30, the definition is in
include/uqhip.h).

`parse(spec)` gives what uq_adapter_mark takes, `explicit(spec)` the canonical form config.json records.  A spec is

    key=value[,key=value...]

    seq=LETTERS|NAME    the adapter: 1..64 letters of ACGT in either case, or a preset name (required)
    seq2=LETTERS|NAME   the second mates' adapter (--mate2 / --interleaved only; without it both mates use seq)
    err=E               mismatches allowed per 100 compared bases, 0..30 (default 10)
    overlap=N           the fewest bases a match at the read's end must hold, 1..64, not above the shorter sequence (default 3)

The presets are Trim Galore's prefixes: illumina = AGATCGGAAGAGC, nextera = CTGTCTCTTATA, smallrna = TGGAATTCTCGG.  The read is cut at the
leftmost position where the adapter, or as much of it as the read still holds, matches with few enough mismatches (Hamming distance, N never
matches); a record whose sequence and quality lines differ in length stays as it is.
"""
from .errors import UqError

MAX_LEN = 64
KEYS = ('seq', 'seq2', 'err', 'overlap')
PRESETS = {'illumina': 'AGATCGGAAGAGC', 'nextera': 'CTGTCTCTTATA', 'smallrna': 'TGGAATTCTCGG'}
DEFAULTS = {'err': 10, 'overlap': 3}
INT_KEYS = {'err': (0, 30), 'overlap': (1, MAX_LEN)}
HELP = ('find a 3\' adapter in every read and cut the read there, on the GPU before encoding (extension).  SPEC is key=value[,key=value...]: '
        'seq=LETTERS (1..64 of ACGT) or a preset name (illumina, nextera, smallrna), seq2= the same for the second mates (--mate2 / --interleaved), '
        'err=E mismatches per 100 compared bases (0..30, default 10), overlap=N bases a match at the read\'s end must hold (default 3).  The leftmost '
        'match wins; mismatches only, no insertions or deletions; sequence and quality lose the same positions.  Runs behind --trim and in front of '
        '--filter and --bin-qual.  The container is the plain encode of the cut reads; config.json records the criteria and the counts.  Encode only')


def _digits(text):
    """ASCII digits only: what int() takes without a surprise (str.isdigit alone also accepts characters such as a superscript two)."""
    return text.isascii() and text.isdigit()


def _bad(spec, why):
    return UqError('ERROR: --adapter %r: %s' % (spec, why))


def items(spec):
    """[(key, value text)] of a spec in the order given: known keys, none twice."""
    if spec is None or not str(spec).strip(): raise UqError('ERROR: --adapter: the specification is empty')
    out, seen = [], set()
    for item in str(spec).split(','):
        if item.count('=') != 1: raise _bad(spec, '%r is not key=value' % item.strip())
        key, value = (part.strip() for part in item.split('='))      # spaces around a key or a value are dropped; inside one they are an error
        if key not in KEYS: raise _bad(spec, 'unknown key %r (keys: %s)' % (key, ', '.join(KEYS)))
        if key in seen: raise _bad(spec, 'the key %r is given twice' % key)
        seen.add(key)
        out.append((key, value))
    return out


def _sequence(spec, key, value):
    """Upper-case letters of a sequence value: a preset's, or the value's own."""
    if value.lower() in PRESETS: return PRESETS[value.lower()]
    letters = value.upper()
    if not letters: raise _bad(spec, '%s= is empty' % key)
    if not (letters.isascii() and all(c in 'ACGT' for c in letters)):
        raise _bad(spec, '%s=%r is neither letters of ACGT nor a preset (%s)' % (key, value, ', '.join(sorted(PRESETS))))
    if len(letters) > MAX_LEN: raise _bad(spec, '%s holds %d letters, at most %d are taken' % (key, len(letters), MAX_LEN))
    return letters


def parse(spec):
    """SPEC -> {'seq', 'seq2' (None when not given), 'err', 'overlap'}: sequences as upper-case letters."""
    c = {'seq': None, 'seq2': None, **DEFAULTS}
    for key, value in items(spec):
        if key in INT_KEYS:
            lo, hi = INT_KEYS[key]
            if not _digits(value): raise _bad(spec, '%s=%r is not a non-negative integer' % (key, value))
            if not lo <= int(value) <= hi: raise _bad(spec, '%s=%s is outside %d..%d' % (key, value, lo, hi))
            c[key] = int(value)
        else:
            c[key] = _sequence(spec, key, value)
    if c['seq'] is None: raise _bad(spec, 'seq= is required')
    shortest = min(len(c[k]) for k in ('seq', 'seq2') if c[k] is not None)
    if c['overlap'] > shortest: raise _bad(spec, 'overlap=%d is above the %d letters of the shorter sequence' % (c['overlap'], shortest))
    return c


def explicit(spec):
    """The canonical form of a spec: presets expanded to upper-case letters, the defaults filled in, in the order seq, seq2, err, overlap; seq2
    only when it was given.  Two specs that mean the same search have the same form."""
    c = parse(spec)
    return ','.join('%s=%s' % (k, c[k]) for k in KEYS if c[k] is not None)


def report_line(report):
    """The one line the analysis prints: how many reads were cut, in full or at their end, and how many bases are left."""
    bi, bo = report['bases_in'], report['bases_out']
    return 'adapter: %d of %d reads cut (%d full, %d partial), %d of %d bases kept (%s %%)' % (
        report['reads_cut'], report['reads_in'], report['full'], report['partial'], bo, bi, ('%.2f' % (100.0 * bo / bi)) if bi else '0.00')
