"""--bin-qual SPEC: the quality bins of a lossy encode (an extension).

`parse(spec)` gives the 256-byte table uq_requantise_qualities applies to every quality line before the encoder looks at the text.
A spec speaks in Phred values with the usual +33 offset (Phred+64 files are out of scope):

    LO-HI:Q[,LO-HI:Q...]    every quality LO..HI becomes Q; `V:Q` is the range V-V; LO <= HI, all values in 0..93, ranges disjoint
    illumina8               3-9:6,10-19:15,20-24:22,25-29:27,30-34:33,35-39:37,40-93:40
    4level                  3-14:12,15-30:23,31-93:37

Bytes outside every range stay as they are, anything that is not in 33..126 included.  Both presets leave Q0, Q1 and Q2 alone: Q2 ('#') is
what Illumina gives a no-call, and an N that keeps a quality of its own keeps the N-trick in its clean form (N is stored as the most popular
base under a quality code nobody else uses: DNA stays at 2 bits per base).  Merged with 3-9, `N` would share its one quality with other
bases: the encoder then still takes N out of the alphabet, but under a NEW quality code, which no decoder maps back -- the
container does not give its reads back (`--verify` says so), and the way out, --notricks, costs 3 bits per base instead of 2 (+50 % on the
DNA table).
"""
from .errors import UqError

OFFSET = 33
QMAX = 93
PRESETS = {
    'illumina8': '3-9:6,10-19:15,20-24:22,25-29:27,30-34:33,35-39:37,40-93:40',
    '4level': '3-14:12,15-30:23,31-93:37',
}
HELP = ('lossy: requantise the quality lines on the GPU before encoding (extension).  SPEC is LO-HI:Q[,LO-HI:Q...] in Phred values with the '
        '+33 offset (Phred+64 files are out of scope): every quality LO..HI becomes Q, V:Q is a single value, values 0..93, ranges disjoint, '
        'everything else stays as it is; or a preset: illumina8 = ' + PRESETS['illumina8'] + '; 4level = ' + PRESETS['4level'] + '.  The presets '
        'leave Q0-Q2 alone: Q2 is what Illumina gives a no-call, and merged with 3-9 an N would share its quality with other bases: the N-trick '
        'then needs a quality code of its own that no decoder maps back (SURVEY.md Q9), and without the trick (--notricks) DNA takes 3 bits '
        'per base instead of 2.  Encode only; config.json records the bins and how many '
        'characters changed')


def explicit(spec):
    """The explicit form of a spec: a preset's ranges, or the spec itself (spaces removed)."""
    if spec is None or not str(spec).strip(): raise UqError('ERROR: --bin-qual: the specification is empty')
    s = ''.join(str(spec).split())
    if ':' not in s:
        if s not in PRESETS:
            raise UqError('ERROR: --bin-qual: unknown preset %r (presets: %s; or LO-HI:Q[,LO-HI:Q...])' % (s, ', '.join(sorted(PRESETS))))
        return PRESETS[s]
    return s


def ranges(spec):
    """[(lo, hi, q)] of a spec, validated, in the order given."""
    def value(text, item):
        if not text.isdigit(): raise UqError('ERROR: --bin-qual: %r in %r is not a Phred value (LO-HI:Q or V:Q, integers)' % (text, item))
        v = int(text)
        if v > QMAX: raise UqError('ERROR: --bin-qual: %d in %r is outside 0..%d' % (v, item, QMAX))
        return v
    out, taken = [], {}
    for item in explicit(spec).split(','):
        if item.count(':') != 1: raise UqError('ERROR: --bin-qual: %r is not LO-HI:Q or V:Q' % item)
        span, q = item.split(':')
        lo, _, hi = span.partition('-')
        lo, q = value(lo, item), value(q, item)
        hi = value(hi, item) if '-' in span else lo
        if lo > hi: raise UqError('ERROR: --bin-qual: %r: LO is larger than HI' % item)
        for v in range(lo, hi + 1):
            if v in taken: raise UqError('ERROR: --bin-qual: the ranges %r and %r overlap at %d' % (taken[v], item, v))
            taken[v] = item
        out.append((lo, hi, q))
    return out


def parse(spec):
    """SPEC -> the 256-byte table: identity except chr(33 + v) -> chr(33 + Q) for every v of a range."""
    lut = bytearray(range(256))
    for lo, hi, q in ranges(spec):
        for v in range(lo, hi + 1): lut[OFFSET + v] = OFFSET + q
    return bytes(lut)
