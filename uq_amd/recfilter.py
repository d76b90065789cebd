"""--filter SPEC: which reads an encode keeps (an extension; DESIGN.md section 27, the definition is in include/uqhip.h).

`parse(spec)` gives the criteria uq_filter_mark takes, `explicit(spec)` the canonical form config.json records.  A spec is

    key=value[,key=value...]

    min-len=N      drop reads shorter than N bases
    max-len=N      drop reads longer than N bases
    max-n=N        drop reads with more than N bases that are N or n
    min-mean-q=Q   drop reads whose mean Phred quality (+33 offset, clamped to 0..93) is below Q, 0..93
    sample=F       keep a deterministic fraction 0 < F <= 1 of the reads (of the pairs, for paired input); 1 switches it off
    seed=S         with sample: another sample of the same size

A pair is kept only when both mates pass.  The fraction is taken exactly from its decimal string: sample_threshold = floor(F * 2^64).
"""
import re
from fractions import Fraction

from .errors import UqError

U32_MAX = 0xFFFFFFFF
INT_KEYS = {'min-len': ('min_len', U32_MAX), 'max-len': ('max_len', U32_MAX), 'max-n': ('max_n', U32_MAX), 'min-mean-q': ('min_mean_q', 93)}
KEYS = ('min-len', 'max-len', 'max-n', 'min-mean-q', 'sample', 'seed')
FLAG_SAMPLE = 1
HELP = ('drop reads on the GPU before encoding (extension).  SPEC is key=value[,key=value...]: min-len=N, max-len=N (bases), max-n=N (bases that '
        'are N), min-mean-q=Q (mean Phred quality, 0..93), sample=F (keep the fraction 0 < F <= 1, deterministic) with seed=S.  With --mate2 / '
        '--interleaved a pair is kept only when both mates pass.  The container is the plain encode of the reads kept; config.json records the '
        'criteria and the counts.  Encode only')


DECIMAL = re.compile(r'(?a)^(\d+\.?\d*|\.\d+)$')


def _digits(text):
    """ASCII digits only: what int() takes without a surprise (str.isdigit alone also accepts characters such as a superscript two)."""
    return text.isascii() and text.isdigit()


def _decimal(text):
    """The canonical spelling of a decimal that DECIMAL matches: no leading zeros, no trailing zeros, no bare point ('0.10' and '.1' -> '0.1')."""
    whole, _, frac = text.partition('.')
    whole, frac = whole.lstrip('0') or '0', frac.rstrip('0')
    return whole + ('.' + frac if frac else '')


def _bad(spec, why):
    return UqError('ERROR: --filter %r: %s' % (spec, why))


def items(spec):
    """[(key, value text)] of a spec in the order given: known keys, none twice."""
    if spec is None or not str(spec).strip(): raise UqError('ERROR: --filter: the specification is empty')
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
    """SPEC -> {'min_len', 'max_len', 'max_n', 'min_mean_q', 'sample_threshold', 'seed', 'flags'}: the fields of uq_filter_params but `unit`."""
    c = {'min_len': 0, 'max_len': U32_MAX, 'max_n': U32_MAX, 'min_mean_q': 0, 'sample_threshold': 0, 'seed': 0, 'flags': 0}
    given = dict(items(spec))
    for key, value in given.items():
        if key in INT_KEYS:
            name, top = INT_KEYS[key]
            if not _digits(value): raise _bad(spec, '%s=%r is not a non-negative integer' % (key, value))
            if int(value) > top: raise _bad(spec, '%s=%s is outside 0..%d' % (key, value, top))
            c[name] = int(value)
        elif key == 'seed':
            if not _digits(value): raise _bad(spec, 'seed=%r is not a non-negative integer' % value)
            if int(value) >= 1 << 64: raise _bad(spec, 'seed=%s does not fit 64 bits' % value)
            c['seed'] = int(value)
        else:
            if not DECIMAL.match(value): raise _bad(spec, 'sample=%r is not a decimal fraction (digits with at most one point)' % value)
            f = Fraction(value)
            if not 0 < f <= 1: raise _bad(spec, 'sample=%s is outside 0 < f <= 1' % value)
            if f < 1:
                c['sample_threshold'] = int(f * (1 << 64))      # floor: f * 2^64 is an exact rational
                c['flags'] |= FLAG_SAMPLE
    if 'seed' in given and 'sample' not in given: raise _bad(spec, 'seed only goes with sample')
    if c['min_len'] > c['max_len']: raise _bad(spec, 'min-len %d is larger than max-len %d' % (c['min_len'], c['max_len']))
    return c


def explicit(spec):
    """The canonical form of a spec: the keys given, in the order of KEYS, spaces removed, integers and the sample's decimal without leading or
    trailing zeros: two specs that mean the same criteria have the same form."""
    parse(spec)
    given = dict(items(spec))
    return ','.join('%s=%s' % (k, _decimal(given[k]) if k == 'sample' else int(given[k])) for k in KEYS if k in given)


def report_line(report):
    """The one line the analysis prints: how many reads were kept, and what dropped the others."""
    n, kept = report['reads_in'], report['reads_out']
    by = ', '.join('%s %d' % (k, report['fail_' + k]) for k in ('min_len', 'max_len', 'max_n', 'mean_q', 'sample', 'mate'))
    return 'filter: kept %d of %d reads (%s %%), by criterion: %s' % (kept, n, ('%.2f' % (100.0 * kept / n)) if n else '0.00', by)
