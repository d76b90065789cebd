"""--dedup SPEC: which reads count as duplicates of an earlier one and are dropped (an extension; DESIGN.md section 32, the definition is in
include/uqhip.h).

`parse(spec)` gives the criteria uq_dedup_keys takes, `explicit(spec)` the canonical form config.json records.  A spec is

    key=value[,key=value...]

    by=seq         compare the sequence lines (the only value: it makes the bare form spellable)
    prefix=N       compare the first N bases of every read only; 0, the default, compares whole reads
    keep=first     of equal reads keep the first in input order (the default)
    keep=best      ... the one whose qualities sum highest (Phred, +33 offset, clamped to 0..93), ties to the earlier read

Reads are equal when their compared bases are the same bytes: case-sensitive, N equals N.  A pair is a duplicate only when both mates are.
"""
from .errors import UqError

U32_MAX = 0xFFFFFFFF
KEYS = ('by', 'prefix', 'keep')
KEEP = {'first': 0, 'best': 1}
FLAG_BEST = 1
HELP = ('drop duplicate reads on the GPU before encoding (extension).  SPEC is key=value[,key=value...]: by=seq (compare the sequence lines; the '
        'only value), prefix=N (compare the first N bases only; 0 = whole reads), keep=first|best (of equal reads keep the first, or the one with '
        'the highest quality sum).  Exact: reads are compared byte for byte, a hash only finds the candidates.  With --mate2 / --interleaved a pair '
        'is dropped only when both mates repeat an earlier pair.  Runs behind --trim, --adapter and --filter, in front of --bin-qual.  The container '
        'is the plain encode of the reads kept; config.json records the criteria and the counts.  Encode only')


def _digits(text):
    """ASCII digits only: what int() takes without a surprise (str.isdigit alone also accepts characters such as a superscript two)."""
    return text.isascii() and text.isdigit()


def _bad(spec, why):
    return UqError('ERROR: --dedup %r: %s' % (spec, why))


def items(spec):
    """[(key, value text)] of a spec in the order given: known keys, none twice."""
    if spec is None or not str(spec).strip(): raise UqError('ERROR: --dedup: the specification is empty')
    out, seen = [], set()
    for item in str(spec).split(','):
        if item.count('=') != 1: raise _bad(spec, '%r is not key=value' % item.strip())
        key, value = (part.strip() for part in item.split('='))      # spaces around a key or a value are dropped; inside one they are an error
        if key not in KEYS: raise _bad(spec, 'unknown key %r (keys: %s)' % (key, ', '.join(KEYS)))
        if key in seen: raise _bad(spec, 'the key %r is given twice' % key)
        seen.add(key)
        out.append((key, value))
    return out


def parse(spec):
    """SPEC -> {'prefix', 'flags'}: the fields of uq_dedup_params but `unit`, `hash_bits` and `seed`."""
    c = {'prefix': 0, 'flags': 0}
    for key, value in items(spec):
        if key == 'by':
            if value != 'seq': raise _bad(spec, 'by=%r: the only value is seq' % value)
        elif key == 'prefix':
            if not _digits(value): raise _bad(spec, 'prefix=%r is not a non-negative integer' % value)
            if int(value) > U32_MAX: raise _bad(spec, 'prefix=%s is outside 0..%d' % (value, U32_MAX))
            c['prefix'] = int(value)
        else:
            if value not in KEEP: raise _bad(spec, 'keep=%r is neither first nor best' % value)
            if KEEP[value]: c['flags'] |= FLAG_BEST
    return c


def explicit(spec):
    """The canonical form of a spec: every key, in the order of KEYS, spaces removed, the integer without leading zeros: two specs that mean
    the same criteria have the same form."""
    c = parse(spec)
    return 'by=seq,prefix=%d,keep=%s' % (c['prefix'], 'best' if c['flags'] & FLAG_BEST else 'first')


def report_line(report):
    """The one line the analysis prints: how many reads were kept, and how many distinct sequences there are."""
    n, kept = report['reads_in'], report['reads_in'] - report['dup_reads']
    return 'dedup: kept %d of %d reads (%s %% duplicates), %d distinct sequences' % (
        kept, n, ('%.2f' % (100.0 * report['dup_reads'] / n)) if n else '0.00', report['classes'])
