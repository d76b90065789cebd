"""--trim SPEC: which ends an encode cuts off its reads (an extension; DESIGN.md section 28, the definition is in include/uqhip.h).

`parse(spec)` gives the steps uq_trim_mark takes, `explicit(spec)` the canonical form config.json records.  A spec is

    key=value[,key=value...]

    head=N      cut the first N bases
    tail=N      cut the last N bases
    crop=N      then keep at most N bases, N >= 1
    polyg=G     cut a run of G or more G at the 3' end (the dark cycles of two-colour chemistry), G >= 1
    q5=Q        cut the 5' end by the running sum of Q - quality (BWA / cutadapt), 1..93
    q3=Q        the same at the 3' end
    trim-n=1    cut N from both ends

The steps run in that order, whatever the order of the keys; a record whose sequence and quality lines differ in length stays as it is.
"""
from .errors import UqError

U32_MAX = 0xFFFFFFFF
# key -> (field, lowest, highest)
INT_KEYS = {'head': ('head', 0, U32_MAX), 'tail': ('tail', 0, U32_MAX), 'crop': ('crop', 1, U32_MAX - 1), 'polyg': ('polyg', 1, U32_MAX),
            'q5': ('q5', 1, 93), 'q3': ('q3', 1, 93), 'trim-n': ('flags', 0, 1)}
KEYS = ('head', 'tail', 'crop', 'polyg', 'q5', 'q3', 'trim-n')
FLAG_N = 1
OFF = {'head': 0, 'tail': 0, 'crop': U32_MAX, 'polyg': 0, 'q5': 0, 'q3': 0, 'flags': 0}
HELP = ('cut the ends of the reads on the GPU before encoding (extension).  SPEC is key=value[,key=value...]: head=N, tail=N (bases cut), crop=N '
        '(bases kept at most), polyg=G (a 3\' run of G or more G), q5=Q, q3=Q (the BWA / cutadapt running sum, 1..93), trim-n=1 (N at both ends), '
        'applied in that order; sequence and quality lose the same positions.  With --mate2 / --interleaved each mate is trimmed on its own.  '
        'Runs in front of --filter and --bin-qual.  The container is the plain encode of the trimmed reads; config.json records the steps and the '
        'counts.  Encode only')


def _digits(text):
    """ASCII digits only: what int() takes without a surprise (str.isdigit alone also accepts characters such as a superscript two)."""
    return text.isascii() and text.isdigit()


def _bad(spec, why):
    return UqError('ERROR: --trim %r: %s' % (spec, why))


def items(spec):
    """[(key, value text)] of a spec in the order given: known keys, none twice."""
    if spec is None or not str(spec).strip(): raise UqError('ERROR: --trim: the specification is empty')
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
    """SPEC -> {'head', 'tail', 'crop', 'polyg', 'q5', 'q3', 'flags'}: the fields of uq_trim_params."""
    c = dict(OFF)
    for key, value in items(spec):
        name, lo, hi = INT_KEYS[key]
        if not _digits(value): raise _bad(spec, '%s=%r is not a non-negative integer' % (key, value))
        if not lo <= int(value) <= hi: raise _bad(spec, '%s=%s is outside %d..%d' % (key, value, lo, hi))
        c[name] = int(value) * FLAG_N if key == 'trim-n' else int(value)
    if c == OFF: raise _bad(spec, 'it switches no step on')
    return c


def explicit(spec):
    """The canonical form of a spec: the keys given, in the order of KEYS, spaces and leading zeros removed: two specs that mean the same steps
    and name the same keys have the same form."""
    parse(spec)
    given = dict(items(spec))
    return ','.join('%s=%d' % (k, int(given[k])) for k in KEYS if k in given)


def report_line(report):
    """The one line the analysis prints: how many reads were cut, how many bases are left, and which step took the others."""
    n, cut, bi, bo = report['reads_in'], report['reads_trimmed'], report['bases_in'], report['bases_out']
    by = ', '.join('%s %d' % (k, report['cut_' + k]) for k in ('fixed', 'polyg', 'q5', 'q3', 'n'))
    return 'trim: %d of %d reads cut, %d of %d bases kept (%s %%), by step: %s' % (cut, n, bo, bi, ('%.2f' % (100.0 * bo / bi)) if bi else '0.00', by)
